// vf_engine_scorer.inc - host side of the frame scorer (vf_frame_scorer.h; include/vf_hip.h "Learned-cost planning"):
// tensor table, buffers, the launch sequence.  Included at the end of vf_engine.hip (it reads the resident predictions of a
// vf_handle), after vf_engine_sidenet.inc (allocation, upload, weight packing, also under -DVF_HOST_SELFTEST).

struct vf_scorer {
    vf_scorer_config cfg;
    int H = 0, W = 0, ncam = 1, D = 2, towers = 1;
    int group = 0;                      // frame-views per pass through the activation workspace
    float *act[4] = {nullptr};          // outputs of c1 .. c4 for `group` frame-views
    struct Tower {
        int cin = 3;
        size_t blob_floats = 0;         // canonical floats per view
        float *w1 = nullptr, *b1 = nullptr;             // c1 as in the blob, [ncam][9 * cin * 32], [ncam][32]
        float *wp[3] = {nullptr}, *b[3] = {nullptr};    // c2 .. c4 packed for vf_net_conv.h, biases
        float *wfc = nullptr, *bfc = nullptr;           // [ncam][128][D], [ncam][D]
        bool loaded = false;
    } tower[2];
    float *enc = nullptr;               // head outputs of the last pass [max_frames][ncam][D]
    double *raw = nullptr;              // [max_frames] raw cost per (sequence, step)
    std::vector<AllocRec> allocs;
};

namespace vf {

static size_t scorer_act_floats(int H, int W, int layer) {          // layer 1..4: one frame's output of c<layer>
    return (size_t)(H >> layer) * (W >> layer) * kScCh[layer];
}

static int scorer_validate(const vf_scorer_config *cfg) {
    if (!cfg) return fail(VF_ERR_INVALID, "null scorer config");
    if (cfg->height < 16 || cfg->width < 16 || cfg->height % 16 || cfg->width % 16)
        return fail(VF_ERR_INVALID, "scorer height and width must be multiples of 16");
    if (cfg->width > 128) return fail(VF_ERR_INVALID, "scorer width must be at most 128 (the staged rows of c1 stay within 64 KiB of LDS)");
    if (cfg->ncam < 0 || cfg->ncam > 4) return fail(VF_ERR_INVALID, "scorer ncam must be 1..4");
    if (cfg->head != 0 && cfg->head != 1) return fail(VF_ERR_INVALID, "scorer head must be 0 (classifier) or 1 (embedding)");
    if (cfg->head == 1 && (cfg->embed_dim < 1 || cfg->embed_dim > 1024))
        return fail(VF_ERR_INVALID, "scorer embed_dim must be 1..1024");
    if (cfg->max_frames < 1) return fail(VF_ERR_INVALID, "scorer max_frames must be at least 1");
    if (!(cfg->input_scale > 0.f)) return fail(VF_ERR_INVALID, "scorer input_scale must be positive");
    return VF_OK;
}

static size_t scorer_blob_floats(int cin, int D) {
    size_t n = 0;
    int c_in = cin;
    for (int l = 1; l <= 4; ++l) { n += (size_t)9 * c_in * kScCh[l] + kScCh[l]; c_in = kScCh[l]; }
    return n + (size_t)kScCh[4] * D + D;
}

// the refusals of vf_scorer_scores / vf_scorer_embed (host work only: shared by the device build and the host self-test)
static int scorer_scores_check(const vf_scorer *s, const vf_handle *h, const float *d_goal_enc, const double *d_scores) {
    if (!s || !h || !d_scores) return fail(VF_ERR_INVALID, "null argument");
    if (s->H != h->H || s->W != h->W) return fail(VF_ERR_INVALID, "scorer and handle differ in image size");
    if (s->ncam != h->ncam) return fail(VF_ERR_INVALID, "scorer and handle differ in ncam");
    if (s->cfg.device != h->cfg.device) return fail(VF_ERR_INVALID, "scorer and handle live on different devices");
    if (!s->tower[0].loaded) return fail(VF_ERR_INVALID, "scorer weights not loaded");
    if (s->cfg.head == 1 && !d_goal_enc) return fail(VF_ERR_INVALID, "the embedding head needs d_goal_enc");
    if (h->last_B < 1) return fail(VF_ERR_INVALID, "the handle has not rolled");
    return VF_OK;
}

static int scorer_embed_check(const vf_scorer *s, int32_t tower, const float *d_images, int32_t n, const float *d_out) {
    if (!s || !d_images || !d_out) return fail(VF_ERR_INVALID, "null argument");
    if (tower < 0 || tower >= s->towers) return fail(VF_ERR_INVALID, "tower " + std::to_string(tower) + " does not exist");
    if (!s->tower[tower].loaded) return fail(VF_ERR_INVALID, "scorer weights not loaded");
    if (n < 1 || n > s->cfg.max_frames)
        return fail(VF_ERR_INVALID, "n = " + std::to_string(n) + " images, max_frames = " + std::to_string(s->cfg.max_frames));
    if (reinterpret_cast<uintptr_t>(d_images) % 16) return fail(VF_ERR_INVALID, "the images must be 16-byte aligned");
    return VF_OK;
}

#ifndef VF_HOST_SELFTEST
// n_fv frame-views (index = image * ncam + view) of `src` through tower `tw` -> s->enc [n_fv][D]
static int scorer_run(vf_scorer *s, int tw, const ScorerSrc &src, long long n_fv, hipStream_t st) {
    const vf_scorer::Tower &t = s->tower[tw];
    const int H = s->H, W = s->W, D = s->D;
    const size_t lds = ((size_t)(2 * kScBand + 1) * W * t.cin + (size_t)9 * t.cin * kScCh[1]) * sizeof(float);
    for (long long f0 = 0; f0 < n_fv; f0 += s->group) {
        const int n = (int)std::min<long long>(s->group, n_fv - f0);
        const unsigned c1_blocks = (unsigned)n * (unsigned)(H / 2 / kScBand);
        if (t.cin == 3)
            hipLaunchKernelGGL(scorer_c1_kernel<3>, dim3(c1_blocks), dim3(kScThreads), lds, st, src, (int)f0, H, W,
                               s->cfg.input_scale, t.w1, t.b1, (long long)9 * 3 * kScCh[1], s->act[0]);
        else
            hipLaunchKernelGGL(scorer_c1_kernel<6>, dim3(c1_blocks), dim3(kScThreads), lds, st, src, (int)f0, H, W,
                               s->cfg.input_scale, t.w1, t.b1, (long long)9 * 6 * kScCh[1], s->act[0]);
        VF_HIP_CHECK(hipGetLastError());
        for (int l = 2; l <= 4; ++l) {
            const int Hin = H >> (l - 1), Win = W >> (l - 1), Cin = kScCh[l - 1], Cout = kScCh[l];
            const int P = (Hin / 2) * (Win / 2), mtiles = (P + 31) / 32;
            const long long stride = (long long)packed_floats(Cin, Cout);
            if (l == 2)             // NT = 2: all 64 output channels in one wave
                launch_net_conv(scorer_conv_kernel<2>, n, mtiles, 1, st, s->act[0], n, (int)f0, s->ncam, Hin, Win, Cin, Cout,
                                t.wp[0], t.b[0], stride, s->act[1]);
            else                    // NT = 1: four waves share a row tile (few positions are left, more tasks keep the CUs busy)
                launch_net_conv(scorer_conv_kernel<1>, n, mtiles, Cout / 32, st, s->act[l - 2], n, (int)f0, s->ncam, Hin, Win,
                                Cin, Cout, t.wp[l - 2], t.b[l - 2], stride, s->act[l - 1]);
            VF_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(scorer_head_kernel, dim3((unsigned)n), dim3(kScHeadThreads), 0, st, s->act[3], (int)f0, s->ncam,
                           (H / 16) * (W / 16), D, t.wfc, t.bfc, s->enc);
        VF_HIP_CHECK(hipGetLastError());
    }
    return VF_OK;
}
#endif

}  // namespace vf

extern "C" {

size_t vf_scorer_weight_count(const vf_scorer_config *cfg, int32_t tower) {
    VF_API_TRY
    if (scorer_validate(cfg)) return 0;
    if (tower < 0 || tower > cfg->head) { fail(VF_ERR_INVALID, "tower " + std::to_string(tower) + " does not exist"); return 0; }
    return scorer_blob_floats(tower == 1 ? 6 : 3, cfg->head == 1 ? cfg->embed_dim : 2);
    VF_API_CATCH(size_t)
}

int vf_scorer_destroy(vf_scorer *s) {
    VF_API_TRY
    if (!s) return VF_OK;
    side_free_all(s->cfg.device, s->allocs);
    delete s;
    return VF_OK;
    VF_API_CATCH(int)
}

int vf_scorer_create(const vf_scorer_config *cfg, vf_scorer **out) {
    vf_scorer *made = nullptr;     // (released if anything below throws)
    VF_API_TRY
    if (!out) return fail(VF_ERR_INVALID, "null out pointer");
    *out = nullptr;
    int rc = scorer_validate(cfg);
    if (rc) return rc;
#ifndef VF_HOST_SELFTEST
    VF_HIP_CHECK(hipSetDevice(cfg->device));
#endif
    vf_scorer *s = new vf_scorer();
    made = s;
    s->cfg = *cfg;
    s->H = cfg->height; s->W = cfg->width;
    s->ncam = std::max(1, cfg->ncam);
    s->cfg.ncam = s->ncam;
    s->D = cfg->head == 1 ? cfg->embed_dim : 2;
    s->towers = cfg->head == 1 ? 2 : 1;
    size_t per_frame = 0;
    for (int l = 1; l <= 4; ++l) per_frame += scorer_act_floats(s->H, s->W, l);
    // the activations of a pass stay within 256 MB (the last-level cache); the pass size is invisible in the results
    const long long total = (long long)cfg->max_frames * s->ncam;
    s->group = (int)std::max<long long>(1, std::min<long long>(total, ((long long)1 << 28) / (long long)(per_frame * sizeof(float))));
    for (int l = 1; l <= 4; ++l)
        VF_SIDE_ALLOC(s, vf_scorer_destroy, s->act[l - 1], (size_t)s->group * scorer_act_floats(s->H, s->W, l));
    for (int tw = 0; tw < s->towers; ++tw) {
        vf_scorer::Tower &t = s->tower[tw];
        t.cin = tw == 1 ? 6 : 3;
        t.blob_floats = scorer_blob_floats(t.cin, s->D);
        VF_SIDE_ALLOC(s, vf_scorer_destroy, t.w1, (size_t)s->ncam * 9 * t.cin * kScCh[1]);
        VF_SIDE_ALLOC(s, vf_scorer_destroy, t.b1, (size_t)s->ncam * kScCh[1]);
        for (int l = 2; l <= 4; ++l) {
            VF_SIDE_ALLOC(s, vf_scorer_destroy, t.wp[l - 2], s->ncam * packed_floats(kScCh[l - 1], kScCh[l]));
            VF_SIDE_ALLOC(s, vf_scorer_destroy, t.b[l - 2], (size_t)s->ncam * kScCh[l]);
        }
        VF_SIDE_ALLOC(s, vf_scorer_destroy, t.wfc, (size_t)s->ncam * kScCh[4] * s->D);
        VF_SIDE_ALLOC(s, vf_scorer_destroy, t.bfc, (size_t)s->ncam * s->D);
    }
    VF_SIDE_ALLOC(s, vf_scorer_destroy, s->enc, (size_t)total * s->D);
    VF_SIDE_ALLOC(s, vf_scorer_destroy, s->raw, (size_t)cfg->max_frames);
    VF_INJECT(4);
    *out = s;
    return VF_OK;
    VF_API_CATCH_CLEANUP(int, { if (made) vf_scorer_destroy(made); if (out) *out = nullptr; })
}

int vf_scorer_load_weights(vf_scorer *s, int32_t tower, const float *host_blob, size_t n_floats) {
    VF_API_TRY
    if (!s || !host_blob) return fail(VF_ERR_INVALID, "null scorer or blob");
    if (tower < 0 || tower >= s->towers) return fail(VF_ERR_INVALID, "tower " + std::to_string(tower) + " does not exist");
    vf_scorer::Tower &t = s->tower[tower];
    const size_t want = t.blob_floats * s->ncam;
    if (n_floats != want)
        return fail(VF_ERR_INVALID, "scorer weight blob has " + std::to_string(n_floats) + " floats, expected " + std::to_string(want));
    VF_INJECT(5);
#ifndef VF_HOST_SELFTEST
    VF_HIP_CHECK(hipSetDevice(s->cfg.device));
    VF_HIP_CHECK(hipDeviceSynchronize());       // (hot swap: passes in flight have finished)
#endif
    for (int v = 0; v < s->ncam; ++v) {
        BlobCursor blob{host_blob + (size_t)v * t.blob_floats, v};
        blob.upload(t.w1, (size_t)9 * t.cin * kScCh[1]);
        blob.upload(t.b1, kScCh[1]);
        for (int l = 2; l <= 4; ++l) {
            blob.upload_packed(t.wp[l - 2], kScCh[l - 1], kScCh[l]);
            blob.upload(t.b[l - 2], kScCh[l]);
        }
        blob.upload(t.wfc, (size_t)kScCh[4] * s->D);
        blob.upload(t.bfc, s->D);
        if (blob.rc) return blob.rc;
    }
    t.loaded = true;
    return VF_OK;
    VF_API_CATCH(int)
}

#ifdef VF_HOST_SELFTEST
int vf_scorer_embed(vf_scorer *s, int32_t tower, const float *d_images, int32_t n, float *d_out, void *) {
    VF_API_TRY                                  // (refusal paths only: this build launches nothing)
    if (int rc = scorer_embed_check(s, tower, d_images, n, d_out)) return rc;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
    VF_API_CATCH(int)
}
int vf_scorer_scores(vf_scorer *s, vf_handle *h, const float *d_goal_enc, float, double *d_scores, double *, float *, void *) {
    VF_API_TRY
    if (int rc = scorer_scores_check(s, h, d_goal_enc, d_scores)) return rc;
    return fail(VF_ERR_HIP, "the host self-test build launches nothing");
    VF_API_CATCH(int)
}
#else
int vf_scorer_embed(vf_scorer *s, int32_t tower, const float *d_images, int32_t n, float *d_out, void *stream) {
    VF_API_TRY
    if (int rc = scorer_embed_check(s, tower, d_images, n, d_out)) return rc;
    VF_HIP_CHECK(hipSetDevice(s->cfg.device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long img = (long long)s->H * s->W * s->tower[tower].cin;
    const ScorerSrc src = {d_images, img, img * s->ncam, s->ncam, 1, 0, 1};
    if (int rc = scorer_run(s, tower, src, (long long)n * s->ncam, st)) return rc;
    VF_HIP_CHECK(hipMemcpyAsync(d_out, s->enc, (size_t)n * s->ncam * s->D * sizeof(float), hipMemcpyDeviceToDevice, st));
    return VF_OK;
    VF_API_CATCH(int)
}

int vf_scorer_scores(vf_scorer *s, vf_handle *h, const float *d_goal_enc, float finalweight, double *d_scores,
                     double *d_cost_per_step, float *d_head_out, void *stream) {
    VF_API_TRY
    if (int rc = scorer_scores_check(s, h, d_goal_enc, d_scores)) return rc;
    const int B = h->last_B, T = h->T, NV = h->ncam;
    // only the steps the cost needs are scored: the last one, unless the weighting or an optional output wants them all
    const bool all_steps = finalweight >= 0.f || d_cost_per_step || d_head_out;
    const int t0 = all_steps ? 0 : T - 1, n_steps = all_steps ? T : 1;
    if ((long long)B * n_steps > s->cfg.max_frames)
        return fail(VF_ERR_INVALID, std::to_string((long long)B * n_steps) + " frames per view exceed max_frames = " +
                                        std::to_string(s->cfg.max_frames));
    VF_HIP_CHECK(hipSetDevice(s->cfg.device));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long long img = (long long)h->H * h->W * 3;
    const ScorerSrc src = {h->frames_all, (long long)h->cfg.max_batch * T * img, img, NV, T, t0, n_steps};
    const long long n_img = (long long)B * n_steps;
    if (int rc = scorer_run(s, 0, src, n_img * NV, st)) return rc;
    hipLaunchKernelGGL(scorer_raw_cost_kernel, dim3((unsigned)((n_img + 63) / 64)), dim3(64), 0, st, s->enc, d_goal_enc, (int)n_img,
                       NV, s->D, s->cfg.head, s->raw);
    VF_HIP_CHECK(hipGetLastError());
    const int n_actions = B / h->n_draws;
    // (finalweight < 0 with every step scored: the kernel reads the last of its n_steps columns)
    hipLaunchKernelGGL(scorer_scores_kernel, dim3((unsigned)((n_actions + 63) / 64)), dim3(64), 0, st, s->raw, n_actions,
                       h->n_draws, n_steps, finalweight, h->d_status, d_scores, d_cost_per_step);
    VF_HIP_CHECK(hipGetLastError());
    if (d_head_out) {
        const long long n = n_img * NV * s->D;
        hipLaunchKernelGGL(scorer_copy_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s->enc, n, h->d_status,
                           d_head_out);
        VF_HIP_CHECK(hipGetLastError());
    }
    return VF_OK;
    VF_API_CATCH(int)
}
#endif

}  // extern "C"
