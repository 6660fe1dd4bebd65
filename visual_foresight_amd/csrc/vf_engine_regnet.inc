// vf_engine_regnet.inc - host side of the registration network (vf_registration_net.h; include/vf_hip.h "Registration
// network"): tensor table, buffers, the launch sequence.  Included at the end of vf_engine.hip, after vf_engine_sidenet.inc
// (allocation, upload, weight packing, also under -DVF_HOST_SELFTEST).

struct vf_regnet {
    vf_regnet_config cfg;
    int H = 0, W = 0, ncam = 1, m = 1, n_img = 0;      // n_img = max_pairs * ncam
    size_t blob_floats = 0;                             // canonical floats per view
    float *w1 = nullptr, *b1 = nullptr;                 // d1 as in the blob, [ncam][54 * 32m], [ncam][32m]
    float *wp[5] = {nullptr}, *b[5] = {nullptr};        // d2, d3, u1, u2, u3 packed for vf_net_conv.h, biases
    float *wf = nullptr, *bf = nullptr;                 // flow head [ncam][25 * 16m * 2], [ncam][2]
    float *down[3] = {nullptr};                         // outputs of d1 .. d3 (pooled)
    float *conv = nullptr;                              // output of the convolution of u1 .. u3 before up-sampling
    float *up[3] = {nullptr};                           // outputs of u1 .. u3 (up-sampled)
    bool loaded = false;
    std::vector<AllocRec> allocs;
};

namespace vf {

// the five matrix-pipe layers: input / output channels per m, the divisor of the size the convolution runs at, pooling
struct RegnetConvLayer { int cin, cout, div; bool pool; };
static const RegnetConvLayer kRnConv[5] = {{32, 64, 2, true}, {64, 128, 4, true}, {128, 64, 8, false}, {64, 32, 4, false},
                                           {32, 16, 2, false}};

static int regnet_validate(const vf_regnet_config *cfg) {
    if (!cfg) return fail(VF_ERR_INVALID, "null registration-net config");
    if (cfg->height < 16 || cfg->width < 16 || cfg->height % 8 || cfg->width % 8)
        return fail(VF_ERR_INVALID, "registration-net height and width must be multiples of 8 and at least 16");
    if (cfg->height > kRnMaxSize || cfg->width > kRnMaxSize)
        return fail(VF_ERR_INVALID, "registration-net height and width must be at most 128");
    if (cfg->ncam < 0 || cfg->ncam > 4) return fail(VF_ERR_INVALID, "registration-net ncam must be 1..4");
    if (cfg->ch_mult != 1 && cfg->ch_mult != 2 && cfg->ch_mult != 4)
        return fail(VF_ERR_INVALID, "registration-net ch_mult must be 1, 2 or 4");
    if (cfg->max_pairs < 1 || cfg->max_pairs > 4096) return fail(VF_ERR_INVALID, "registration-net max_pairs must be 1..4096");
    return VF_OK;
}

static size_t regnet_blob_floats(int m) {
    size_t n = (size_t)54 * 32 * m + 32 * m;
    for (const RegnetConvLayer &l : kRnConv) n += (size_t)9 * l.cin * m * l.cout * m + l.cout * m;
    return n + (size_t)25 * 16 * m * 2 + 2;
}

// the refusals of vf_regnet_flow (host work only: shared by the device build and the host self-test)
static int regnet_flow_check(const vf_regnet *r, const float *d_current, const float *d_reference, int32_t n, const float *d_flow) {
    if (!r || !d_current || !d_reference || !d_flow) return fail(VF_ERR_INVALID, "null argument");
    if (!r->loaded) return fail(VF_ERR_INVALID, "registration-net weights not loaded");
    if (n < 1 || n > r->cfg.max_pairs)
        return fail(VF_ERR_INVALID, "n = " + std::to_string(n) + " pairs, max_pairs = " + std::to_string(r->cfg.max_pairs));
    if (reinterpret_cast<uintptr_t>(d_current) % 16 || reinterpret_cast<uintptr_t>(d_reference) % 16)
        return fail(VF_ERR_INVALID, "the images must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_flow) % 8) return fail(VF_ERR_INVALID, "the flow field must be 8-byte aligned");
    return VF_OK;
}

#ifndef VF_HOST_SELFTEST
template <bool POOL>
static void regnet_launch_conv(const float *in, int n_img, int ncam, int Hin, int Win, int Cin, int Cout, const float *wp,
                               const float *bias, float *out, hipStream_t st) {
    // 16-column tiles unless the map is narrower than wide tiles can fill; pooling needs them
    const int tw_shift = (POOL || Win % 16 == 0) ? 4 : 3;
    const int tw = 1 << tw_shift, th = 32 >> tw_shift;
    const long long mtiles = (long long)((Win + tw - 1) / tw) * ((Hin + th - 1) / th);
    const int ntile = (Cout + 31) / 32;
    const long long stride = (long long)packed_floats(Cin, Cout);
    // two channel tiles per wave share the activation loads where one image alone still yields a wave per SIMD and more
    // (the choice depends on the layer's shape only, and no output value's summation order depends on it).  Pooling layers
    // only: no other layer of a configuration regnet_validate accepts reaches the condition.
    if (POOL && ntile % 2 == 0 && mtiles * (ntile / 2) >= 256)
        launch_net_conv(regnet_conv_kernel<2, true>, n_img, mtiles, ntile / 2, st, in, n_img, ncam, Hin, Win, Cin, Cout, tw_shift,
                        wp, bias, stride, out);
    else
        launch_net_conv(regnet_conv_kernel<1, POOL>, n_img, mtiles, ntile, st, in, n_img, ncam, Hin, Win, Cin, Cout, tw_shift,
                        wp, bias, stride, out);
}

static int regnet_run(vf_regnet *r, const float *d_current, const float *d_reference, int n, float *d_flow, hipStream_t st) {
    const int H = r->H, W = r->W, m = r->m, NV = r->ncam, n_img = n * NV;
    const size_t lds1 = ((size_t)2 * (2 * kRnBand + 2) * W * 3 + 54 * 32) * sizeof(float);
    hipLaunchKernelGGL(regnet_d1_kernel, dim3((unsigned)(n_img * (H / 2 / kRnBand) * m)), dim3(kRnThreads), lds1, st, d_current,
                       d_reference, NV, H, W, 32 * m, r->w1, r->b1, r->down[0]);
    VF_HIP_CHECK(hipGetLastError());
    for (int l = 0; l < 5; ++l) {
        const RegnetConvLayer &L = kRnConv[l];
        const int Hin = H / L.div, Win = W / L.div, Cin = L.cin * m, Cout = L.cout * m;
        const float *in = l < 3 ? r->down[l] : r->up[l - 3];
        if (L.pool) {
            regnet_launch_conv<true>(in, n_img, NV, Hin, Win, Cin, Cout, r->wp[l], r->b[l], r->down[l + 1], st);
            VF_HIP_CHECK(hipGetLastError());
        } else {
            regnet_launch_conv<false>(in, n_img, NV, Hin, Win, Cin, Cout, r->wp[l], r->b[l], r->conv, st);
            VF_HIP_CHECK(hipGetLastError());
            const long long n4 = (long long)n_img * 2 * Hin * 2 * Win * (Cout / 4);
            hipLaunchKernelGGL(regnet_upsample_kernel, dim3((unsigned)((n4 + kRnThreads - 1) / kRnThreads)), dim3(kRnThreads), 0, st,
                               r->conv, n4, Hin, Win, Cout, r->up[l - 2]);
            VF_HIP_CHECK(hipGetLastError());
        }
    }
    const int Cf = 16 * m;
    hipLaunchKernelGGL(regnet_flow_kernel, dim3((unsigned)((long long)n_img * H * W / kRnFlowThreads)), dim3(kRnFlowThreads),
                       (size_t)25 * Cf * 2 * sizeof(float), st, r->up[2], NV, H, W, Cf, r->wf, r->bf, d_flow);
    VF_HIP_CHECK(hipGetLastError());
    return VF_OK;
}
#endif

}  // namespace vf

extern "C" {

size_t vf_regnet_weight_count(const vf_regnet_config *cfg) {
    VF_API_TRY
    if (regnet_validate(cfg)) return 0;
    return regnet_blob_floats(cfg->ch_mult);
    VF_API_CATCH(size_t)
}

int vf_regnet_destroy(vf_regnet *r) {
    VF_API_TRY
    if (!r) return VF_OK;
    side_free_all(r->cfg.device, r->allocs);
    delete r;
    return VF_OK;
    VF_API_CATCH(int)
}

int vf_regnet_create(const vf_regnet_config *cfg, vf_regnet **out) {
    vf_regnet *made = nullptr;     // (released if anything below throws)
    VF_API_TRY
    if (!out) return fail(VF_ERR_INVALID, "null out pointer");
    *out = nullptr;
    int rc = regnet_validate(cfg);
    if (rc) return rc;
#ifndef VF_HOST_SELFTEST
    VF_HIP_CHECK(hipSetDevice(cfg->device));
#endif
    vf_regnet *r = new vf_regnet();
    made = r;
    r->cfg = *cfg;
    r->H = cfg->height; r->W = cfg->width; r->m = cfg->ch_mult;
    r->ncam = std::max(1, cfg->ncam);
    r->cfg.ncam = r->ncam;
    r->n_img = cfg->max_pairs * r->ncam;
    r->blob_floats = regnet_blob_floats(r->m);
    const int m = r->m, NV = r->ncam;
    const size_t HW = (size_t)r->H * r->W, N = (size_t)r->n_img;
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->w1, (size_t)NV * 54 * 32 * m);
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->b1, (size_t)NV * 32 * m);
    for (int l = 0; l < 5; ++l) {
        const int Cin = kRnConv[l].cin * m, Cout = kRnConv[l].cout * m;
        VF_SIDE_ALLOC(r, vf_regnet_destroy, r->wp[l], NV * packed_floats(Cin, Cout));
        VF_SIDE_ALLOC(r, vf_regnet_destroy, r->b[l], (size_t)NV * Cout);
    }
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->wf, (size_t)NV * 25 * 16 * m * 2);
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->bf, (size_t)NV * 2);
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->down[0], N * (HW / 4) * 32 * m);
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->down[1], N * (HW / 16) * 64 * m);
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->down[2], N * (HW / 64) * 128 * m);
    // (the largest of u1 (HW / 64 * 64m), u2 (HW / 16 * 32m), u3 (HW / 4 * 16m))
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->conv, N * (HW / 4) * 16 * m);
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->up[0], N * (HW / 16) * 64 * m);
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->up[1], N * (HW / 4) * 32 * m);
    VF_SIDE_ALLOC(r, vf_regnet_destroy, r->up[2], N * HW * 16 * m);
    *out = r;
    return VF_OK;
    VF_API_CATCH_CLEANUP(int, { if (made) vf_regnet_destroy(made); if (out) *out = nullptr; })
}

int vf_regnet_load_weights(vf_regnet *r, const float *host_blob, size_t n_floats) {
    VF_API_TRY
    if (!r || !host_blob) return fail(VF_ERR_INVALID, "null registration net or blob");
    const size_t want = r->blob_floats * r->ncam;
    if (n_floats != want)
        return fail(VF_ERR_INVALID, "registration-net weight blob has " + std::to_string(n_floats) + " floats, expected " +
                                        std::to_string(want));
#ifndef VF_HOST_SELFTEST
    VF_HIP_CHECK(hipSetDevice(r->cfg.device));
    VF_HIP_CHECK(hipDeviceSynchronize());       // (hot swap: calls in flight have finished)
#endif
    const int m = r->m;
    for (int v = 0; v < r->ncam; ++v) {
        BlobCursor blob{host_blob + (size_t)v * r->blob_floats, v};
        blob.upload(r->w1, (size_t)54 * 32 * m);
        blob.upload(r->b1, 32 * m);
        for (int l = 0; l < 5; ++l) {
            blob.upload_packed(r->wp[l], kRnConv[l].cin * m, kRnConv[l].cout * m);
            blob.upload(r->b[l], kRnConv[l].cout * m);
        }
        blob.upload(r->wf, (size_t)25 * 16 * m * 2);
        blob.upload(r->bf, 2);
        if (blob.rc) return blob.rc;
    }
    r->loaded = true;
    return VF_OK;
    VF_API_CATCH(int)
}

int vf_regnet_flow(vf_regnet *r, const float *d_current, const float *d_reference, int32_t n, float *d_flow, void *stream) {
    VF_API_TRY
    if (int rc = regnet_flow_check(r, d_current, d_reference, n, d_flow)) return rc;
#ifdef VF_HOST_SELFTEST
    (void)stream;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
#else
    VF_HIP_CHECK(hipSetDevice(r->cfg.device));
    return regnet_run(r, d_current, d_reference, n, d_flow, reinterpret_cast<hipStream_t>(stream));
#endif
    VF_API_CATCH(int)
}

}  // extern "C"
