// host_selftest_grouped.cc - grouped contexts (vf_set_contexts) in the ASan/UBSan CPU build of the engine's
// host side (see host_selftest.cc: vf_engine.hip compiled for the HOST ONLY with -DVF_HOST_SELFTEST, device allocations are
// address reservations, nothing is launched).  In grouped mode step_io points the context inputs of every step at per-row
// buffers with row strides and a view offset of `rows` rows; vf_selftest_schedule re-checks every pointer of every phase of
// such a schedule - `(B - 1) * stride + span` of each - against the handle's allocations, which hold the grouped buffers
// from the first vf_set_contexts on.  Cases: one and two views, one to three context frames, every compositing table,
// frames-only, batches below and at max_batch; then the refusals, and the way back to the broadcast context.
// Never built for or run on a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vf_hip.h"

extern "C" int vf_set_fuse_top(vf_handle *h, int32_t enable);
extern "C" int vf_selftest_schedule(vf_handle *h, int32_t B, int32_t skip_shared, int64_t *out_items,
                                    uint64_t *out_upload_checksum);

static int g_fail = 0;
#define EXPECT(cond, what)                                                                              \
    do {                                                                                                \
        if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s (%s)\n", __LINE__, what, vf_last_error()); ++g_fail; } \
    } while (0)

static vf_handle *make(int H, int W, int nd, int nctx, int T, int max_batch, int ncam, int layer_spec, int arch = 0,
                       int n_draws = 1) {
    const int num_masks = arch == 2 ? 6 : (arch == 0 && layer_spec == 3 ? 1 : 10);
    vf_config cfg = {H, W, 4, 5, nd, nctx, nctx + T, num_masks, max_batch, 0, 0, ncam, n_draws, arch, 0, layer_spec};
    const size_t n = vf_weight_count(&cfg);
    vf_handle *h = nullptr;
    if (n == 0 || vf_create(&cfg, &h)) { std::fprintf(stderr, "vf_create failed: %s\n", vf_last_error()); return nullptr; }
    std::vector<float> blob(n * (size_t)ncam);
    uint32_t s = 777u + (uint32_t)(H + W + ncam);
    for (float &x : blob) { s = s * 1664525u + 1013904223u; x = ((float)(s >> 8) / 16777216.0f - 0.5f) * 0.2f; }
    if (vf_load_weights(h, blob.data(), blob.size())) { std::fprintf(stderr, "vf_load_weights failed: %s\n", vf_last_error()); return nullptr; }
    return h;
}

// the caller's context arrays are never read by this build: any non-null address stands for them
static const uint8_t *const kFrames = reinterpret_cast<const uint8_t *>(0x1000);
static const float *const kFloats = reinterpret_cast<const float *>(0x2000);

static bool names_grouped() { return std::strstr(vf_last_error(), "grouped contexts") != nullptr; }

// G groups of m rows on a handle of max_batch rows: the schedule of the grouped rollout passes, fused and unfused top,
// and differs from the broadcast schedule of the same batch exactly as a schedule without shared units does
static void grouped_case(int H, int W, int nd, int nctx, int T, int max_batch, int ncam, int layer_spec, int G, int m) {
    vf_handle *h = make(H, W, nd, nctx, T, max_batch, ncam, layer_spec);
    EXPECT(h != nullptr, "create");
    if (!h) return;
    const int B = G * m;
    int64_t broadcast = 0, grouped = 0, again = 0;
    uint64_t sum = 0;
    EXPECT(vf_selftest_schedule(h, B, 0, &broadcast, &sum) == 0, "broadcast schedule");
    const float *distrib = nd > 0 ? kFloats : nullptr;
    EXPECT(vf_set_contexts(h, G, m, kFrames, kFloats, kFloats, distrib, nullptr) == 0, "vf_set_contexts");
    for (int fuse = 1; fuse >= 0; --fuse) {
        vf_set_fuse_top(h, fuse);
        EXPECT(vf_selftest_schedule(h, B, 0, &grouped, &sum) == 0, "grouped schedule");
    }
    vf_set_fuse_top(h, 1);
    EXPECT(vf_selftest_schedule(h, B, 0, &grouped, &sum) == 0, "grouped schedule");
    // nothing is shared between the rows: never fewer items than the de-duplicated schedule
    EXPECT(grouped >= broadcast, "a grouped schedule shares nothing");
    // a second call changes the grouping and allocates nothing new that the check could miss
    EXPECT(vf_set_contexts(h, 1, B, kFrames, kFloats, kFloats, distrib, nullptr) == 0, "one group");
    EXPECT(vf_selftest_schedule(h, B, 0, &again, &sum) == 0 && again == grouped, "one group of B rows: the same schedule");
    // back to the broadcast context: the schedule of before
    EXPECT(vf_set_context(h, kFrames, kFloats, kFloats, distrib, nullptr) == 0, "vf_set_context");
    EXPECT(vf_selftest_schedule(h, B, 0, &again, &sum) == 0 && again == broadcast, "broadcast schedule after grouped mode");
    std::printf("  grouped %dx%d nd %d nctx %d ncam %d spec %d  %d x %d of %d rows: %lld items (broadcast %lld)\n", H, W, nd, nctx,
                ncam, layer_spec, G, m, max_batch, (long long)grouped, (long long)broadcast);
    vf_destroy(h);
}

static void refusals() {
    vf_handle *h = make(32, 32, 1, 2, 2, 6, 1, 0);
    EXPECT(h != nullptr, "create");
    if (!h) return;
    double scores[6];
    const int32_t *goal = reinterpret_cast<const int32_t *>(0x3000);
    EXPECT(vf_group_pixel_scores(h, goal, 10.f, nullptr, scores, nullptr, nullptr) == VF_ERR_INVALID && names_grouped(),
           "cost outside grouped mode");
    const struct { int G, m; bool frames, actions, distrib; } bad[] = {
        {0, 3, true, true, true}, {2, 0, true, true, true}, {-1, 3, true, true, true}, {2, 4, true, true, true},
        {2, 3, false, true, true}, {2, 3, true, false, true}, {2, 3, true, true, false}};
    for (const auto &b : bad) {
        EXPECT(vf_set_contexts(h, b.G, b.m, b.frames ? kFrames : nullptr, kFloats, b.actions ? kFloats : nullptr,
                               b.distrib ? kFloats : nullptr, nullptr) == VF_ERR_INVALID && names_grouped(), "bad vf_set_contexts accepted");
        EXPECT(vf_group_pixel_scores(h, goal, 10.f, nullptr, scores, nullptr, nullptr) == VF_ERR_INVALID, "still broadcast");
    }
    EXPECT(vf_set_contexts(nullptr, 2, 3, kFrames, kFloats, kFloats, kFloats, nullptr) == VF_ERR_INVALID, "null handle");
    EXPECT(vf_set_contexts(h, 2, 3, kFrames, kFloats, kFloats, kFloats, nullptr) == 0, "vf_set_contexts");
    // grouped, but nothing has rolled since
    EXPECT(vf_group_pixel_scores(h, goal, 10.f, nullptr, scores, nullptr, nullptr) == VF_ERR_INVALID && names_grouped() &&
               std::strstr(vf_last_error(), "not rolled"), "cost before a rollout");
    EXPECT(vf_group_pixel_scores(h, nullptr, 10.f, nullptr, scores, nullptr, nullptr) == VF_ERR_INVALID, "null goals");
    EXPECT(vf_group_pixel_scores(h, goal, 10.f, nullptr, nullptr, nullptr, nullptr) == VF_ERR_INVALID, "null scores");
    vf_destroy(h);
    // a frames-only handle takes no distributions and has no grouped pixel cost
    h = make(32, 32, 0, 2, 2, 6, 1, 0);
    EXPECT(h != nullptr, "create frames-only");
    if (h) {
        EXPECT(vf_set_contexts(h, 2, 3, kFrames, kFloats, kFloats, kFloats, nullptr) == VF_ERR_INVALID && names_grouped(), "frames-only with distributions");
        EXPECT(vf_set_contexts(h, 2, 3, kFrames, kFloats, kFloats, nullptr, nullptr) == 0, "frames-only");
        EXPECT(vf_group_pixel_scores(h, goal, 10.f, nullptr, scores, nullptr, nullptr) == VF_ERR_INVALID && names_grouped(), "frames-only cost");
        vf_destroy(h);
    }
    // other architectures and latent draws
    for (int arch = 1; arch <= 2; ++arch) {
        h = make(64, 64, 1, 2, 2, 6, 1, 0, arch);
        EXPECT(h != nullptr, "create arch 1 / 2");
        if (!h) continue;
        EXPECT(vf_set_contexts(h, 2, 3, kFrames, kFloats, kFloats, kFloats, nullptr) == VF_ERR_INVALID && names_grouped() &&
                   std::strstr(vf_last_error(), "arch"), "arch 1 / 2 accepted");
        vf_destroy(h);
    }
    h = make(32, 32, 1, 2, 2, 6, 1, 0, 0, 2);
    EXPECT(h != nullptr, "create n_draws 2");
    if (h) {
        EXPECT(vf_set_contexts(h, 2, 3, kFrames, kFloats, kFloats, kFloats, nullptr) == VF_ERR_INVALID && names_grouped() &&
                   std::strstr(vf_last_error(), "n_draws"), "n_draws 2 accepted");
        vf_destroy(h);
    }
}

int main() {
    // (H, W, nd, nctx, T, max_batch, ncam, layer_spec, G, m): batches below max_batch and at it, one and two views
    grouped_case(32, 32, 1, 2, 3, 37, 1, 0, 3, 7);
    grouped_case(32, 32, 1, 2, 3, 21, 1, 0, 3, 7);
    grouped_case(40, 56, 2, 1, 2, 16, 1, 0, 2, 8);
    grouped_case(48, 64, 1, 3, 2, 16, 1, 0, 5, 1);
    grouped_case(32, 32, 0, 2, 2, 16, 1, 0, 2, 3);
    grouped_case(32, 32, 1, 2, 2, 37, 2, 0, 2, 3);
    grouped_case(40, 56, 4, 2, 2, 16, 2, 0, 2, 8);
    grouped_case(64, 64, 1, 2, 13, 200, 1, 0, 8, 25);
    for (int spec = 1; spec <= 4; ++spec) {
        grouped_case(32, 32, 1, 2, 3, 37, 1, spec, 3, 7);
        grouped_case(40, 56, 2, 2, 2, 37, 2, spec, 2, 8);
    }
    refusals();
    if (g_fail) { std::printf("HOST SELFTEST (grouped contexts) FAILED: %d\n", g_fail); return 1; }
    std::printf("HOST SELFTEST (grouped contexts) OK\n");
    return 0;
}
