// host_selftest.cc - driver of the ASan/UBSan CPU build of the engine's host-side code
// ("build the C-ABI lib with an ASan/UBSan CPU variant").
//
// vf_engine.hip is compiled for the HOST ONLY with -DVF_HOST_SELFTEST: device allocations become
// address reservations, uploads become checksums.  What runs under the sanitizers is exactly the
// product's host code: the tensor table, the layer planner, the weight packers (fp32 and
// split-bf16), the rollout emitter and the persistent-schedule builder - for several shapes,
// view counts, batch sizes and both schedule variants - and vf_selftest_schedule() checks the
// invariants the device relies on (contiguous tickets, dependencies on earlier phases only,
// counters in range, every pointer of every phase inside a buffer of the handle).
// Never built for or run on a GPU (GPU sanitizers are not available on this pool).
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vf_hip.h"

extern "C" int vf_set_fuse_top(vf_handle *h, int32_t enable);
extern "C" int vf_selftest_inject(int32_t where, int32_t kind);
extern "C" int vf_selftest_schedule(vf_handle *h, int32_t B, int32_t skip_shared, int64_t *out_items,
                                    uint64_t *out_upload_checksum);

static int run_case(int H, int W, int adim, int sdim, int nd, int nctx, int T, int max_batch, int precision, int ncam,
                    int n_draws, const int *batches, int n_batches, int arch = 0, int zdim = 0, int layer_spec = 0) {
    const int num_masks = arch == 3 ? 4 : (arch == 2 ? 6 : (arch == 0 && layer_spec == 3 ? 1 : 10));     // (DNA: one transform)
    vf_config cfg = {H, W, adim, sdim, nd, nctx, nctx + T, num_masks, max_batch, 0, precision, ncam, n_draws, arch,
                     zdim, layer_spec};
    const size_t n = vf_weight_count(&cfg);
    if (n == 0) { std::fprintf(stderr, "weight count failed: %s\n", vf_last_error()); return 1; }
    std::vector<float> blob(n * (size_t)ncam);
    uint32_t s = 12345u + (uint32_t)(H * 7 + W * 3 + adim + ncam);
    for (float &x : blob) { s = s * 1664525u + 1013904223u; x = ((float)(s >> 8) / 16777216.0f - 0.5f) * 0.2f; }
    vf_handle *h = nullptr;
    if (vf_create(&cfg, &h)) { std::fprintf(stderr, "vf_create failed: %s\n", vf_last_error()); return 1; }
    if (vf_load_weights(h, blob.data(), blob.size()) != 0 ||
        vf_load_weights(h, blob.data(), blob.size()) != 0) {            // a reload reuses the same buffers
        std::fprintf(stderr, "vf_load_weights failed: %s\n", vf_last_error());
        return 1;
    }
    if (vf_load_weights(h, blob.data(), blob.size() - 1) == 0) { std::fprintf(stderr, "short blob accepted\n"); return 1; }
    uint64_t sum = 0;
    for (int fuse = 1; fuse >= 0; --fuse) {
      vf_set_fuse_top(h, fuse);        // fused decoder top, then the two-phase top
      for (int i = 0; i < n_batches; ++i)
        for (int skip = 0; skip < 2; ++skip) {
            int64_t items = 0;
            if (vf_selftest_schedule(h, batches[i], skip, &items, &sum)) {
                std::fprintf(stderr, "schedule B=%d skip=%d: %s\n", batches[i], skip, vf_last_error());
                return 1;
            }
            std::printf("  %dx%d adim %d nd %d ncam %d prec %d  B=%-4d %s%s: %lld items\n", H, W, adim, nd, ncam,
                        precision, batches[i], skip ? "cached-context" : "full", fuse ? "" : " (unfused top)",
                        (long long)items);
        }
    }
    std::printf("  packed-weight checksum %016llx\n", (unsigned long long)sum);
    vf_destroy(h);
    return 0;
}

int main() {
    const int b_small[] = {1, 7, 16, 37};
    const int b_c2[] = {200, 125, 25};
    const int b_c3[] = {600, 88};
    const int b_c5[] = {50, 5};
    int rc = 0;
    rc |= run_case(32, 32, 4, 5, 1, 2, 3, 37, 0, 1, 1, b_small, 4);
    rc |= run_case(48, 64, 3, 3, 2, 2, 2, 37, 1, 1, 1, b_small, 4);
    rc |= run_case(64, 64, 4, 5, 1, 1, 2, 16, 0, 1, 1, b_small, 3);
    rc |= run_case(64, 64, 4, 5, 1, 2, 13, 200, 0, 1, 1, b_c2, 3);
    rc |= run_case(64, 64, 4, 5, 1, 1, 2, 200, 0, 1, 1, b_c2, 3);    // one context frame at batches that take the 64- / 128-row plans
    rc |= run_case(64, 64, 4, 5, 2, 2, 13, 600, 0, 2, 1, b_c3, 2);
    rc |= run_case(128, 128, 12, 5, 1, 2, 15, 50, 1, 1, 5, b_c5, 2);
    rc |= run_case(40, 56, 5, 5, 4, 2, 2, 16, 0, 3, 1, b_small, 3);
    // arch 1: the SAVP-class four-scale generator (config 5 shard and a small odd shape)
    rc |= run_case(128, 128, 12, 5, 1, 2, 15, 125, 0, 1, 5, b_c2 + 1, 2, 1);
    rc |= run_case(48, 80, 6, 3, 2, 2, 2, 37, 1, 2, 1, b_small, 4, 1);
    // arch 2: arch 1 + the conditioning vector in every conv-LSTM (PH_COND items) + the seven-layer compositing
    rc |= run_case(128, 128, 12, 5, 1, 2, 15, 125, 0, 1, 5, b_c2 + 1, 2, 2);
    rc |= run_case(64, 80, 6, 3, 2, 2, 2, 37, 0, 2, 1, b_small, 4, 2);
    rc |= run_case(64, 64, 12, 5, 3, 1, 2, 16, 0, 1, 1, b_small, 3, 2);
    // arch 0 on the decoder widths of the public CDNA code (layer_spec 1: convt2 96 -> 96, convt3 64 -> 64, unfused top)
    rc |= run_case(64, 64, 4, 5, 2, 2, 3, 37, 0, 1, 1, b_small, 4, 0, 0, 1);
    rc |= run_case(48, 64, 3, 3, 1, 2, 13, 200, 0, 2, 1, b_c2, 3, 0, 0, 1);
    // arch 0 with appearance-flow compositing (layer_spec 2: no CDNA FC, no kernel-finish items; fused and two-phase top, the
    // shape that cannot be fused, four designated pixels, two views) - and, first, the cdna table of the first flow shape:
    // the two may differ by exactly the FC and finish items (tests/test_appflow.py)
    rc |= run_case(64, 64, 7, 5, 2, 2, 3, 37, 0, 1, 1, b_small, 4, 0, 0, 0);
    rc |= run_case(64, 64, 7, 5, 2, 2, 3, 37, 0, 1, 1, b_small, 4, 0, 0, 2);
    rc |= run_case(32, 32, 7, 5, 1, 1, 2, 16, 0, 1, 1, b_small, 3, 0, 0, 2);
    rc |= run_case(40, 56, 7, 5, 4, 2, 2, 16, 0, 2, 1, b_small, 3, 0, 0, 2);
    rc |= run_case(64, 64, 7, 3, 1, 2, 13, 200, 0, 1, 1, b_c2, 3, 0, 0, 2);
    // arch 3: the published SAVP generator - every layer table (32 / 64 / 128 pixels, the paper's table forced on 128 x 128),
    // a config-5 shard, two views, an odd shape
    rc |= run_case(32, 32, 12, 5, 1, 2, 3, 37, 0, 1, 1, b_small, 4, 3, 8);
    rc |= run_case(64, 64, 12, 5, 2, 2, 3, 37, 0, 2, 1, b_small, 4, 3, 8);
    rc |= run_case(48, 64, 6, 3, 4, 1, 2, 16, 0, 1, 1, b_small, 3, 3, 2);
    rc |= run_case(128, 128, 12, 5, 1, 2, 15, 125, 0, 1, 5, b_c2 + 1, 2, 3, 8);
    rc |= run_case(128, 128, 12, 5, 1, 2, 4, 10, 0, 1, 5, b_c5 + 1, 1, 3, 8, 64);
    // arch 0 with DNA compositing (layer_spec 3, num_masks 1: a 5x5 kernel per pixel from a 1x1 head - no CDNA FC, no
    // kernel-finish items, no kernel table): a fusable shape, the shape that cannot be fused (two views, four designated
    // pixels), one context frame, a planning-size batch - each behind the cdna table of the same shape, from which it may
    // differ by exactly the FC and finish items (tests/test_dna.py).  Appended behind every other shape, under shape lines of
    // their own (adim 5), so that the rows the other tests count and index stay where they are.
    for (int spec : {0, 3}) rc |= run_case(64, 64, 5, 5, 2, 2, 3, 37, 0, 1, 1, b_small, 4, 0, 0, spec);
    for (int spec : {0, 3}) rc |= run_case(40, 56, 5, 5, 4, 2, 2, 16, 0, 2, 1, b_small, 3, 0, 0, spec);
    for (int spec : {0, 3}) rc |= run_case(32, 32, 5, 5, 1, 1, 2, 16, 0, 1, 1, b_small, 3, 0, 0, spec);
    for (int spec : {0, 3}) rc |= run_case(64, 64, 5, 3, 1, 2, 13, 200, 0, 1, 1, b_c2, 3, 0, 0, spec);
    // arch 0 with STP compositing (layer_spec 4, num_masks 10: nine affine warps per sample from a two-layer FC head - the
    // first layer on the CDNA FC's plan, one PH_STP_FIN item per sample, a table of transforms where the kernel table sits;
    // the self-test refuses such a schedule without the finish dependency, without the table, or with a flow / dna head or a
    // CDNA kernel-finish item): the four shapes of the DNA block, each behind the cdna table of the same shape, from which
    // its item count does not differ - the same K splits of the FC and one finish item per sample (tests/test_stp.py).
    // Appended behind every other shape, under shape lines of their own (adim 9).
    for (int spec : {0, 4}) rc |= run_case(64, 64, 9, 5, 2, 2, 3, 37, 0, 1, 1, b_small, 4, 0, 0, spec);
    for (int spec : {0, 4}) rc |= run_case(40, 56, 9, 5, 4, 2, 2, 16, 0, 2, 1, b_small, 3, 0, 0, spec);
    for (int spec : {0, 4}) rc |= run_case(32, 32, 9, 5, 1, 1, 2, 16, 0, 1, 1, b_small, 3, 0, 0, spec);
    for (int spec : {0, 4}) rc |= run_case(64, 64, 9, 3, 1, 2, 13, 200, 0, 1, 1, b_c2, 3, 0, 0, spec);
    // invalid configurations are refused, not crashed on
    vf_config bad = {60, 64, 4, 5, 1, 2, 15, 10, 8, 0, 0, 1, 1, 0};
    vf_handle *h = nullptr;
    if (vf_create(&bad, &h) == 0) { std::fprintf(stderr, "invalid config accepted\n"); rc = 1; }
    vf_config bad2 = {64, 64, 4, 5, 1, 2, 15, 10, 8, 0, 0, 5, 1, 0};
    if (vf_create(&bad2, &h) == 0) { std::fprintf(stderr, "ncam 5 accepted\n"); rc = 1; }
    vf_config bad3 = {72, 64, 4, 5, 1, 2, 15, 10, 8, 0, 0, 1, 1, 1};       // arch 1 needs multiples of 16
    if (vf_create(&bad3, &h) == 0) { std::fprintf(stderr, "arch 1 at 72x64 accepted\n"); rc = 1; }
    vf_config bad4 = {64, 64, 12, 5, 1, 2, 15, 10, 8, 0, 0, 1, 1, 2};      // arch 2 composes four warps: num_masks 6
    if (vf_create(&bad4, &h) == 0) { std::fprintf(stderr, "arch 2 with num_masks 10 accepted\n"); rc = 1; }
    vf_config bad5 = {64, 64, 12, 5, 1, 2, 15, 6, 8, 0, 1, 1, 1, 2};       // arch 2 is fp32 only
    if (vf_create(&bad5, &h) == 0) { std::fprintf(stderr, "arch 2 in the split-bf16 mode accepted\n"); rc = 1; }
    vf_config bad6 = {64, 64, 12, 5, 1, 2, 15, 4, 8, 0, 0, 1, 1, 3, 0, 0};     // arch 3 needs zdim
    if (vf_create(&bad6, &h) == 0) { std::fprintf(stderr, "arch 3 without latent channels accepted\n"); rc = 1; }
    vf_config bad7 = {64, 64, 12, 5, 1, 2, 15, 10, 8, 0, 0, 1, 1, 0, 8, 0};    // zdim belongs to arch 3
    if (vf_create(&bad7, &h) == 0) { std::fprintf(stderr, "zdim with arch 0 accepted\n"); rc = 1; }
    vf_config bad8 = {72, 64, 12, 5, 1, 2, 15, 4, 8, 0, 0, 1, 1, 3, 8, 128};   // four scales need multiples of 16
    if (vf_create(&bad8, &h) == 0) { std::fprintf(stderr, "arch 3 / four scales at 72x64 accepted\n"); rc = 1; }
    vf_config bad9 = {64, 64, 4, 5, 1, 2, 15, 10, 8, 0, 1, 1, 1, 0, 0, 2};     // appearance flow is fp32 only
    if (vf_create(&bad9, &h) == 0) { std::fprintf(stderr, "appearance flow in the split-bf16 mode accepted\n"); rc = 1; }
    vf_config bad10 = {128, 128, 12, 5, 1, 2, 15, 10, 8, 0, 0, 1, 1, 1, 0, 2};  // ... and belongs to arch 0
    if (vf_create(&bad10, &h) == 0) { std::fprintf(stderr, "appearance flow with arch 1 accepted\n"); rc = 1; }
    vf_config bad11 = {64, 64, 4, 5, 1, 2, 15, 1, 8, 0, 2, 1, 1, 0, 0, 3};      // DNA is fp32 only
    if (vf_create(&bad11, &h) == 0) { std::fprintf(stderr, "DNA in the plain-bf16 mode accepted\n"); rc = 1; }
    vf_config bad12 = {64, 64, 4, 5, 1, 2, 15, 10, 8, 0, 0, 1, 1, 0, 0, 3};     // ... has one transform
    if (vf_create(&bad12, &h) == 0) { std::fprintf(stderr, "DNA with num_masks 10 accepted\n"); rc = 1; }
    vf_config bad13 = {128, 128, 12, 5, 1, 2, 15, 1, 8, 0, 0, 1, 1, 1, 0, 3};   // ... and belongs to arch 0
    if (vf_create(&bad13, &h) == 0) { std::fprintf(stderr, "DNA with arch 1 accepted\n"); rc = 1; }
    vf_config bad14 = {64, 64, 4, 5, 1, 2, 15, 10, 8, 0, 1, 1, 1, 0, 0, 4};     // STP is fp32 only
    if (vf_create(&bad14, &h) == 0) { std::fprintf(stderr, "STP in the split-bf16 mode accepted\n"); rc = 1; }
    vf_config bad15 = {64, 64, 4, 5, 1, 2, 15, 1, 8, 0, 0, 1, 1, 0, 0, 4};      // ... has nine transforms
    if (vf_create(&bad15, &h) == 0) { std::fprintf(stderr, "STP with num_masks 1 accepted\n"); rc = 1; }
    vf_config bad16 = {128, 128, 12, 5, 1, 2, 15, 10, 8, 0, 0, 1, 1, 1, 0, 4};  // ... and belongs to arch 0
    if (vf_create(&bad16, &h) == 0) { std::fprintf(stderr, "STP with arch 1 accepted\n"); rc = 1; }
    vf_config bad17 = {64, 64, 4, 5, 1, 2, 15, 10, 8, 0, 0, 1, 1, 0, 0, 5};     // no fifth table
    if (vf_create(&bad17, &h) == 0) { std::fprintf(stderr, "layer_spec 5 accepted\n"); rc = 1; }
    // "No exception crosses this boundary" (include/vf_hip.h): a std::bad_alloc / std::exception / foreign throw inside the
    // schedule builder, the weight packer or vf_create comes back as a status code with vf_last_error() set, leaks nothing
    // (ASan's leak check runs at exit) and leaves the handle usable and destroyable
    {
        vf_config cfg = {64, 64, 4, 5, 1, 2, 5, 10, 16, 0, 0, 1, 1, 0, 0, 0};
        const size_t n = vf_weight_count(&cfg);
        std::vector<float> blob(n, 0.01f);
        vf_handle *hh = nullptr;
        const int want_code[3] = {VF_ERR_NOMEM, VF_ERR_INVALID, VF_ERR_INVALID};
        const char *want_msg[3] = {"out of memory", "exception: injected failure", "unknown exception"};
        for (int kind = 0; kind < 3; ++kind) {
            vf_selftest_inject(3, kind);
            hh = reinterpret_cast<vf_handle *>(1);
            const int r = vf_create(&cfg, &hh);
            if (r != want_code[kind] || hh != nullptr || std::string(vf_last_error()) != want_msg[kind]) {
                std::fprintf(stderr, "vf_create under injected failure %d: rc %d, '%s'\n", kind, r, vf_last_error()); rc = 1;
            }
        }
        if (vf_create(&cfg, &hh)) { std::fprintf(stderr, "vf_create after the injected failures: %s\n", vf_last_error()); rc = 1; }
        for (int kind = 0; kind < 3 && hh; ++kind) {
            vf_selftest_inject(2, kind);
            int r = vf_load_weights(hh, blob.data(), blob.size());
            if (r != want_code[kind] || std::string(vf_last_error()) != want_msg[kind]) {
                std::fprintf(stderr, "vf_load_weights under injected failure %d: rc %d, '%s'\n", kind, r, vf_last_error()); rc = 1;
            }
            if (vf_load_weights(hh, blob.data(), blob.size())) { std::fprintf(stderr, "reload after failure: %s\n", vf_last_error()); rc = 1; }
            vf_selftest_inject(1, kind);
            int64_t items = 0; uint64_t sum = 0;
            r = vf_selftest_schedule(hh, 7, 0, &items, &sum);
            if (r != want_code[kind] || std::string(vf_last_error()) != want_msg[kind]) {
                std::fprintf(stderr, "build_schedule under injected failure %d: rc %d, '%s'\n", kind, r, vf_last_error()); rc = 1;
            }
            if (vf_selftest_schedule(hh, 7, 0, &items, &sum) || items <= 0) {
                std::fprintf(stderr, "schedule after failure: %s\n", vf_last_error()); rc = 1;
            }
        }
        // vf_goal_image_scores refuses before it touches the device: NULL arguments, a bad steps_mode, a handle that has not rolled
        if (hh) {
            alignas(16) float goal[4];
            double score = 0.0;
            struct { vf_handle *h; const float *g; int mode; double *out; const char *msg; } refusals[] = {
                {nullptr, goal, 0, &score, "null argument"}, {hh, nullptr, 0, &score, "null argument"},
                {hh, goal, 0, nullptr, "null argument"},     {hh, goal, 2, &score, "steps_mode"},
                {hh, goal, -1, &score, "steps_mode"},        {hh, goal, 1, &score, "not rolled"}};
            for (const auto &c : refusals) {
                const int r = vf_goal_image_scores(c.h, c.g, c.mode, 10.f, 0, c.out, nullptr, nullptr, nullptr);
                if (r != VF_ERR_INVALID || std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                    std::fprintf(stderr, "vf_goal_image_scores: want refusal '%s', got rc %d '%s'\n", c.msg, r, vf_last_error()); rc = 1;
                }
            }
        }
        // vf_render_plans likewise: NULL arguments, nothing to render, no colour table, a bad K, a handle that has not rolled
        if (hh) {
            int32_t seq[1] = {0};
            uint8_t lut[768] = {0}, out[4] = {0};
            struct { vf_handle *h; const int32_t *seq; int K; const uint8_t *lut; uint8_t *f, *d; const char *msg; } refusals[] = {
                {nullptr, seq, 1, lut, out, out, "null argument"},  {hh, nullptr, 1, lut, out, out, "null argument"},
                {hh, seq, 1, lut, nullptr, nullptr, "both outputs"}, {hh, seq, 1, nullptr, out, out, "colour table"},
                {hh, seq, 0, lut, out, out, "at least one"},          {hh, seq, 1 << 20, lut, out, nullptr, "max_batch"},
                {hh, seq, 1, nullptr, out, nullptr, "not rolled"}};
            for (const auto &c : refusals) {
                const int r = vf_render_plans(c.h, c.seq, c.K, c.lut, c.f, c.d, nullptr);
                if (r != VF_ERR_INVALID || std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                    std::fprintf(stderr, "vf_render_plans: want refusal '%s', got rc %d '%s'\n", c.msg, r, vf_last_error()); rc = 1;
                }
            }
        }
        // the frame scorer (learned-cost planning): table, buffers and packer for both heads and the three sizes; injected
        // failures in vf_scorer_create / vf_scorer_load_weights; the refusals of vf_scorer_scores / vf_scorer_embed
        {
            const int sizes[3][2] = {{64, 64}, {48, 64}, {128, 128}};
            for (int head = 0; head < 2; ++head)
                for (const auto &sz : sizes) {
                    vf_scorer_config sc = {sz[0], sz[1], 2, head, 24, 50, 0, head ? 255.f : 1.f};
                    vf_scorer *s = nullptr;
                    if (vf_scorer_create(&sc, &s)) { std::fprintf(stderr, "vf_scorer_create: %s\n", vf_last_error()); rc = 1; continue; }
                    for (int tower = 0; tower <= head; ++tower) {
                        const size_t n = vf_scorer_weight_count(&sc, tower) * 2;
                        std::vector<float> w(n, 0.01f);
                        if (n == 0 || vf_scorer_load_weights(s, tower, w.data(), n) || vf_scorer_load_weights(s, tower, w.data(), n)) {
                            std::fprintf(stderr, "vf_scorer_load_weights: %s\n", vf_last_error()); rc = 1;
                        }
                        if (vf_scorer_load_weights(s, tower, w.data(), n - 1) == 0) { std::fprintf(stderr, "short scorer blob accepted\n"); rc = 1; }
                    }
                    if (vf_scorer_load_weights(s, head + 1, nullptr, 0) == 0) { std::fprintf(stderr, "bad tower accepted\n"); rc = 1; }
                    if (vf_scorer_destroy(s)) rc = 1;
                }
            vf_scorer_config bad_sc = {40, 64, 1, 0, 2, 10, 0, 1.f};
            vf_scorer *s = nullptr;
            if (vf_scorer_create(&bad_sc, &s) == 0 || vf_scorer_weight_count(&bad_sc, 0) != 0) { std::fprintf(stderr, "scorer at 40x64 accepted\n"); rc = 1; }
            vf_scorer_config sc = {64, 64, 1, 1, 16, 100, 0, 255.f};
            for (int kind = 0; kind < 3; ++kind) {
                vf_selftest_inject(4, kind);
                s = reinterpret_cast<vf_scorer *>(1);
                const int r = vf_scorer_create(&sc, &s);
                if (r != want_code[kind] || s != nullptr || std::string(vf_last_error()) != want_msg[kind]) {
                    std::fprintf(stderr, "vf_scorer_create under injected failure %d: rc %d, '%s'\n", kind, r, vf_last_error()); rc = 1;
                }
            }
            if (vf_scorer_create(&sc, &s)) { std::fprintf(stderr, "vf_scorer_create after the injected failures: %s\n", vf_last_error()); rc = 1; s = nullptr; }
            const size_t n0 = vf_scorer_weight_count(&sc, 0);
            std::vector<float> w(n0, 0.01f);
            double score = 0.0;
            alignas(16) float img[4];
            if (s && hh) {
                if (vf_scorer_scores(s, hh, img, 100.f, &score, nullptr, nullptr, nullptr) != VF_ERR_INVALID ||
                    std::string(vf_last_error()).find("not loaded") == std::string::npos) { std::fprintf(stderr, "scores before weights: '%s'\n", vf_last_error()); rc = 1; }
                for (int kind = 0; kind < 3; ++kind) {
                    vf_selftest_inject(5, kind);
                    const int r = vf_scorer_load_weights(s, 0, w.data(), n0);
                    if (r != want_code[kind] || std::string(vf_last_error()) != want_msg[kind]) {
                        std::fprintf(stderr, "vf_scorer_load_weights under injected failure %d: rc %d, '%s'\n", kind, r, vf_last_error()); rc = 1;
                    }
                    if (vf_scorer_load_weights(s, 0, w.data(), n0)) { std::fprintf(stderr, "scorer reload after failure: %s\n", vf_last_error()); rc = 1; }
                }
                struct { vf_scorer *s; vf_handle *h; const float *g; double *out; const char *msg; } refusals[] = {
                    {nullptr, hh, img, &score, "null argument"}, {s, nullptr, img, &score, "null argument"},
                    {s, hh, img, nullptr, "null argument"},      {s, hh, nullptr, &score, "d_goal_enc"},
                    {s, hh, img, &score, "not rolled"}};
                for (const auto &c : refusals) {
                    const int r = vf_scorer_scores(c.s, c.h, c.g, 100.f, c.out, nullptr, nullptr, nullptr);
                    if (r != VF_ERR_INVALID || std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                        std::fprintf(stderr, "vf_scorer_scores: want refusal '%s', got rc %d '%s'\n", c.msg, r, vf_last_error()); rc = 1;
                    }
                }
                vf_scorer_config sc48 = {48, 64, 1, 0, 2, 100, 0, 1.f};
                vf_scorer *s48 = nullptr;
                if (vf_scorer_create(&sc48, &s48) == 0) {
                    if (vf_scorer_scores(s48, hh, nullptr, 100.f, &score, nullptr, nullptr, nullptr) != VF_ERR_INVALID ||
                        std::string(vf_last_error()).find("image size") == std::string::npos) { std::fprintf(stderr, "size mismatch: '%s'\n", vf_last_error()); rc = 1; }
                    vf_scorer_destroy(s48);
                } else rc = 1;
                float out4[4];
                if (vf_scorer_embed(s, 1, img, 1, out4, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("not loaded") == std::string::npos) rc = 1;
                if (vf_scorer_embed(s, 2, img, 1, out4, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("tower") == std::string::npos) rc = 1;
                if (vf_scorer_embed(s, 0, img, 101, out4, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("max_frames") == std::string::npos) rc = 1;
                if (vf_scorer_embed(s, 0, img + 1, 1, out4, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("aligned") == std::string::npos) rc = 1;
                if (vf_scorer_embed(s, 0, nullptr, 1, out4, nullptr) != VF_ERR_INVALID) rc = 1;
            }
            if (s && vf_scorer_destroy(s)) { std::fprintf(stderr, "vf_scorer_destroy failed\n"); rc = 1; }
            std::printf("  frame scorer: both heads at 64x64 / 48x64 / 128x128, injected failures in vf_scorer_create / vf_scorer_load_weights, refusals: %s\n",
                        rc ? "FAILED" : "ok");
        }
        // the registration network: table, buffers and packer (u3 at ch_mult 1 pads 16 channels to a 32-wide tile) for every
        // ch_mult at three sizes, two views; the refusals of vf_regnet_flow
        {
            alignas(16) static float img[8];
            float flow2[2];
            for (int m : {1, 2, 4})
                for (const auto &sz : {std::array<int, 2>{64, 64}, {48, 64}, {128, 128}}) {
                    vf_regnet_config rc_cfg = {sz[0], sz[1], 2, m, 2, 0};
                    vf_regnet *r = nullptr;
                    if (vf_regnet_create(&rc_cfg, &r)) { std::fprintf(stderr, "vf_regnet_create: %s\n", vf_last_error()); rc = 1; continue; }
                    const size_t n = vf_regnet_weight_count(&rc_cfg) * 2;
                    std::vector<float> w(n, 0.5f);
                    if (vf_regnet_flow(r, img, img, 1, flow2, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("not loaded") == std::string::npos) rc = 1;
                    if (n == 0 || vf_regnet_load_weights(r, w.data(), n) || vf_regnet_load_weights(r, w.data(), n)) {
                        std::fprintf(stderr, "vf_regnet_load_weights: %s\n", vf_last_error()); rc = 1;
                    }
                    if (vf_regnet_load_weights(r, w.data(), n - 1) == 0) { std::fprintf(stderr, "short regnet blob accepted\n"); rc = 1; }
                    if (vf_regnet_flow(r, img, img, 3, flow2, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("max_pairs") == std::string::npos) rc = 1;
                    if (vf_regnet_flow(r, img + 1, img, 1, flow2, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("aligned") == std::string::npos) rc = 1;
                    if (vf_regnet_flow(r, img, nullptr, 1, flow2, nullptr) != VF_ERR_INVALID) rc = 1;
                    if (vf_regnet_destroy(r)) rc = 1;
                }
            vf_regnet_config bad_rn = {64, 136, 1, 1, 2, 0};
            vf_regnet *r = nullptr;
            if (vf_regnet_create(&bad_rn, &r) == 0 || vf_regnet_weight_count(&bad_rn) != 0) { std::fprintf(stderr, "regnet at 64x136 accepted\n"); rc = 1; }
            std::printf("  registration net: ch_mult 1 / 2 / 4 at 64x64 / 48x64 / 128x128, refusals: %s\n", rc ? "FAILED" : "ok");
        }
        // the action-inference network of the inverse-model policy: table, buffers and packer (two towers in one buffer per
        // layer) at the ends of every range; the refusals of vf_invmodel_infer
        {
            alignas(16) static float img[8];
            float act[8];
            const int shapes[4][5] = {{16, 16, 1, 1, 1}, {64, 64, 4, 2, 15}, {48, 64, 5, 3, 7}, {96, 128, 8, 4, 32}};
            for (const auto &sh : shapes) {
                vf_invmodel_config ic = {sh[0], sh[1], sh[2], sh[3], sh[4], 2, 0, 1.f};
                vf_invmodel *m = nullptr;
                if (vf_invmodel_create(&ic, &m)) { std::fprintf(stderr, "vf_invmodel_create: %s\n", vf_last_error()); rc = 1; continue; }
                const size_t n = vf_invmodel_weight_count(&ic);
                std::vector<float> w(n, 0.5f);
                if (vf_invmodel_infer(m, img, img, img, act, 1, act, nullptr, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("not loaded") == std::string::npos) rc = 1;
                if (n == 0 || vf_invmodel_load_weights(m, w.data(), n) || vf_invmodel_load_weights(m, w.data(), n)) {
                    std::fprintf(stderr, "vf_invmodel_load_weights: %s\n", vf_last_error()); rc = 1;
                }
                if (vf_invmodel_load_weights(m, w.data(), n - 1) == 0) { std::fprintf(stderr, "short inverse-model blob accepted\n"); rc = 1; }
                if (vf_invmodel_infer(m, img, img, img, act, 3, act, nullptr, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("max_batch") == std::string::npos) rc = 1;
                if (vf_invmodel_infer(m, img, img, img, act, 0, act, nullptr, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_invmodel_infer(m, img + 1, img, img, act, 1, act, nullptr, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("aligned") == std::string::npos) rc = 1;
                if (vf_invmodel_infer(m, img, img, img + 1, act, 1, act, nullptr, nullptr) != VF_ERR_INVALID || std::string(vf_last_error()).find("aligned") == std::string::npos) rc = 1;
                if (vf_invmodel_infer(m, img, nullptr, img, act, 1, act, nullptr, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_invmodel_infer(m, img, img, img, nullptr, 1, act, nullptr, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_invmodel_infer(m, img, img, img, act, 1, nullptr, nullptr, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_invmodel_destroy(m)) rc = 1;
            }
            const vf_invmodel_config bad_im[7] = {{40, 64, 4, 2, 15, 1, 0, 1.f}, {64, 144, 4, 2, 15, 1, 0, 1.f}, {64, 64, 9, 2, 15, 1, 0, 1.f},
                                                  {64, 64, 4, 5, 15, 1, 0, 1.f}, {64, 64, 4, 2, 33, 1, 0, 1.f}, {64, 64, 4, 2, 15, 0, 0, 1.f},
                                                  {64, 64, 4, 2, 15, 1, 0, 0.f}};
            for (const vf_invmodel_config &b : bad_im) {
                vf_invmodel *m = nullptr;
                if (vf_invmodel_create(&b, &m) == 0 || m != nullptr || vf_invmodel_weight_count(&b) != 0) { std::fprintf(stderr, "bad inverse-model config accepted\n"); rc = 1; }
            }
            std::printf("  inverse model: four shapes from 16x16 / adim 1 to 96x128 / adim 8, refusals: %s\n", rc ? "FAILED" : "ok");
        }
        // area resampling and registration at a size of the caller's: the refusals come before the device is touched
        {
            alignas(16) static float img[8];
            void *p = img, *odd = reinterpret_cast<char *>(img) + 2;
            struct { const void *src; void *dst; int dtype, n, Hs, Ws, C, Hd, Wd; const char *msg; } refusals[] = {
                {nullptr, p, 0, 1, 8, 8, 3, 4, 4, "null argument"}, {p, nullptr, 0, 1, 8, 8, 3, 4, 4, "null argument"},
                {p, p, 2, 1, 8, 8, 3, 4, 4, "dtype"},               {p, p, -1, 1, 8, 8, 3, 4, 4, "dtype"},
                {p, p, 0, 0, 8, 8, 3, 4, 4, "n = 0"},               {p, p, 0, 1, 8, 8, 0, 4, 4, "C = 0"},
                {p, p, 0, 1, 8, 8, 5, 4, 4, "C = 5"},               {p, p, 0, 1, 8, 8, 3, 9, 4, "Hd x Wd"},
                {p, p, 1, 1, 8, 8, 3, 4, 9, "Hd x Wd"},             {p, p, 0, 1, 8, 8, 3, 0, 4, "at least 1"},
                {p, p, 0, 1, 2049, 2048, 3, 4, 4, "Hs*Ws"},         {p, p, 0, 1, 1 << 30, 1 << 30, 3, 4, 4, "Hs*Ws"},
                {odd, p, 1, 1, 8, 8, 3, 4, 4, "4-byte aligned"},    {p, odd, 1, 1, 8, 8, 3, 4, 4, "4-byte aligned"},
                {p, p, 0, 1 << 21, 1024, 4, 1, 1024, 4, "n * Hd"},  {p, p, 1, (1 << 30) + 1, 1, 1, 1, 1, 1, "n * Hd"}};
            for (const auto &c : refusals) {
                const int r = vf_resize_area(0, c.src, c.dst, c.dtype, c.n, c.Hs, c.Ws, c.C, c.Hd, c.Wd, nullptr);
                if (r != VF_ERR_INVALID || std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                    std::fprintf(stderr, "vf_resize_area: want refusal '%s', got rc %d '%s'\n", c.msg, r, vf_last_error()); rc = 1;
                }
            }
            if (vf_resize_area(-1, p, p, 0, 1, 8, 8, 3, 4, 4, nullptr) != VF_ERR_INVALID) rc = 1;
            // (an odd uint8 pointer is served: everything is through, and this build launches nothing)
            if (vf_resize_area(0, odd, p, 0, 1, 8, 8, 3, 4, 4, nullptr) != VF_ERR_HIP) { std::fprintf(stderr, "vf_resize_area: odd uint8 pointer refused\n"); rc = 1; }
            // the device CEM entry points: configuration and argument refusals, the workspace size
            {
                const double inf = 1.0 / 0.0;
                vf_cem_config good = {5, 3, 4, 0, 10, 256, 1, 0, 0, 1u, 2u, 0,
                                      {0.075, 0.075, 0.225, inf, inf, inf, inf, inf}, {inf, inf, inf, inf, inf, inf, inf, inf}, {0}};
                if (vf_cem_workspace_bytes(&good) != 16 + 8 * 20 * 21) { std::fprintf(stderr, "vf_cem_workspace_bytes: wrong size\n"); rc = 1; }
                struct { int field, value; const char *msg; } bad_cem[] = {
                    {0, 0, "nactions"}, {0, 33, "exceeds 128"}, {1, 0, "repeat"}, {2, 0, "adim"}, {3, 5, "adim + tail"},
                    {4, 1, "n_elites"}, {4, 257, "n_elites"}, {5, 0, "max_trials"}, {8, 16, "discrete_mask"}};
                for (const auto &c : bad_cem) {
                    vf_cem_config b = good;
                    int32_t words[9];       // the nine leading int32 fields, nactions .. discrete_mask
                    std::memcpy(words, &b, sizeof words);
                    words[c.field] = c.value;
                    std::memcpy(&b, words, sizeof words);
                    if (vf_cem_workspace_bytes(&b) != 0 || std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                        std::fprintf(stderr, "vf_cem_workspace_bytes: want refusal '%s', got '%s'\n", c.msg, vf_last_error()); rc = 1;
                    }
                }
                vf_cem_config neg = good;
                neg.rej_lim[1] = -1.0;
                if (vf_cem_workspace_bytes(&neg) != 0 || vf_cem_workspace_bytes(nullptr) != 0) rc = 1;
                double *pd = reinterpret_cast<double *>(img);
                int32_t *pi = reinterpret_cast<int32_t *>(img);
                if (vf_cem_sample(0, &good, nullptr, 0, 4, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample(0, &good, odd, 0, 4, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample(0, &good, p, 0, 0, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample(0, &good, p, 0, 4097, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample(-1, &good, p, 0, 4, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample(0, &good, p, 0, 4, img, pi, pi, nullptr) != VF_ERR_HIP) rc = 1;      // all through: this build launches nothing
                if (vf_cem_refit(0, &good, pd, img, 9, pi, pd, img, p, nullptr) != VF_ERR_INVALID) rc = 1;     // fewer candidates than elites
                if (vf_cem_refit(0, &good, pd, img, 4097, pi, pd, img, p, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_refit(0, &good, nullptr, img, 10, pi, pd, img, p, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_refit(0, &good, pd, img, 10, pi, pd, img, p, nullptr) != VF_ERR_HIP) rc = 1;
                std::printf("  device CEM: configuration and argument refusals: %s\n", rc ? "FAILED" : "ok");
                // the same for the correlated-noise proposal
                vf_cem_corr_config corr = {10, 4, 0, 20, 0, 0, 1u, 2u, 1.0, 0.5, 0.5,
                                           {0.05, 0.05, 0.2, 0.3}, {0}, {0}, {0}};
                if (vf_cem_corr_workspace_bytes(&corr) != 16 + 8 * (2 * 40 + 20)) { std::fprintf(stderr, "vf_cem_corr_workspace_bytes: wrong size\n"); rc = 1; }
                corr.refit_cov = 1;
                if (vf_cem_corr_workspace_bytes(&corr) != 16 + 8 * (2 * 40 + 20 + 20 * 40)) { std::fprintf(stderr, "vf_cem_corr_workspace_bytes: wrong size with refit_cov\n"); rc = 1; }
                struct { int field, value; const char *msg; } bad_corr[] = {
                    {0, 0, "nactions"}, {0, 33, "exceeds 128"}, {1, 0, "adim"}, {2, 5, "adim + tail"}, {2, -1, "tail"},
                    {3, 1, "n_elites"}, {3, 257, "n_elites"}};
                for (const auto &c : bad_corr) {
                    vf_cem_corr_config b = corr;
                    int32_t words[4];       // the four leading int32 fields, nactions .. n_elites
                    std::memcpy(words, &b, sizeof words);
                    words[c.field] = c.value;
                    std::memcpy(&b, words, sizeof words);
                    if (vf_cem_corr_workspace_bytes(&b) != 0 || std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                        std::fprintf(stderr, "vf_cem_corr_workspace_bytes: want refusal '%s', got '%s'\n", c.msg, vf_last_error()); rc = 1;
                    }
                }
                if (vf_cem_corr_workspace_bytes(nullptr) != 0) rc = 1;
                if (vf_cem_sample_corr(0, &corr, nullptr, 0, 4, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_corr(0, &corr, odd, 0, 4, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_corr(0, &corr, p, 0, 0, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_corr(0, &corr, p, 0, 4097, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_corr(-1, &corr, p, 0, 4, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_corr(0, &corr, p, 0, 4, img, nullptr) != VF_ERR_HIP) rc = 1;         // all through: this build launches nothing
                if (vf_cem_soft_refit(0, &corr, pd, img, 19, pi, pd, img, p, nullptr) != VF_ERR_INVALID) rc = 1;   // fewer candidates than elites
                if (vf_cem_soft_refit(0, &corr, pd, img, 4097, pi, pd, img, p, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_soft_refit(0, &corr, nullptr, img, 20, pi, pd, img, p, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_soft_refit(0, &corr, pd, img, 20, pi, pd, img, odd, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_soft_refit(0, &corr, pd, img, 20, pi, pd, img, p, nullptr) != VF_ERR_HIP) rc = 1;
                std::printf("  device CEM, correlated noise: configuration and argument refusals: %s\n", rc ? "FAILED" : "ok");
                // the same for the folding proposal (its workspace and refit are vf_cem_config's)
                vf_cem_fold_config fold = {5, 3, 0, 10, 2, 0, 1u, 2u, {0.9, 0.1}, {0.2, 0.2, 1.0 / 3}, {0}};
                struct { int field, value; const char *msg; } bad_fold[] = {
                    {0, 4, "nactions"}, {0, 33, "nactions"}, {1, 0, "repeat"}, {2, 5, "tail"}, {2, -1, "tail"},
                    {3, 1, "n_elites"}, {3, 257, "n_elites"}, {4, 0, "n_scripted"}, {4, 10, "n_scripted"}};
                for (const auto &c : bad_fold) {
                    vf_cem_fold_config b = fold;
                    int32_t words[5];       // the five leading int32 fields, nactions .. n_scripted
                    std::memcpy(words, &b, sizeof words);
                    words[c.field] = c.value;
                    std::memcpy(&b, words, sizeof words);
                    if (vf_cem_sample_fold(0, &b, p, 0, 18, img, nullptr) != VF_ERR_INVALID ||
                        std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                        std::fprintf(stderr, "vf_cem_sample_fold: want refusal '%s', got '%s'\n", c.msg, vf_last_error()); rc = 1;
                    }
                }
                if (vf_cem_sample_fold(0, nullptr, p, 0, 18, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_fold(0, &fold, nullptr, 0, 18, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_fold(0, &fold, odd, 0, 18, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_fold(0, &fold, p, 0, 3, img, nullptr) != VF_ERR_INVALID) rc = 1;          // 2 * n_scripted > M
                if (vf_cem_sample_fold(0, &fold, p, 0, 4097, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_fold(-1, &fold, p, 0, 18, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_fold(0, &fold, p, 0, 18, img, nullptr) != VF_ERR_HIP) rc = 1;         // all through: this build launches nothing
                std::printf("  device CEM, folding: configuration and argument refusals: %s\n", rc ? "FAILED" : "ok");
                // the same for the autograsp proposal: the moves' vf_cem_config with the gripper column leading the tail
                vf_cem_config ag = good;
                ag.adim = 3; ag.tail = 1;
                vf_cem_grip_config grip = {0, 0, 0.25, 1.0, 0.15, 0.0, 1.0, -1.0};
                struct { int adim, tail, mode; double dev; int M; const char *msg; } bad_ag[] = {
                    {2, 1, 0, 0.0, 4, "move channels"}, {3, 0, 0, 0.0, 4, "gripper column"}, {3, 6, 0, 0.0, 4, "adim + tail"},
                    {3, 1, 2, 0.0, 4, "mode"}, {3, 1, 0, -0.5, 4, "deviation_prob"}, {3, 1, 0, 1.5, 4, "deviation_prob"},
                    {3, 1, 0, inf - inf, 4, "deviation_prob"}, {3, 1, 0, 0.0, 0, "M = 0"}, {3, 1, 0, 0.0, 4097, "M = 4097"}};
                for (const auto &c : bad_ag) {
                    vf_cem_config b = ag;
                    vf_cem_grip_config g = grip;
                    b.adim = c.adim; b.tail = c.tail; g.mode = c.mode; g.deviation_prob = c.dev;
                    if (vf_cem_sample_autograsp(0, &b, &g, p, 0, c.M, nullptr, nullptr, img, pi, pi, nullptr) != VF_ERR_INVALID ||
                        std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                        std::fprintf(stderr, "vf_cem_sample_autograsp: want refusal '%s', got '%s'\n", c.msg, vf_last_error()); rc = 1;
                    }
                }
                vf_cem_grip_config by_share = grip;
                by_share.mode = 1;
                if (vf_cem_sample_autograsp(0, nullptr, &grip, p, 0, 4, nullptr, nullptr, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_autograsp(0, &ag, nullptr, p, 0, 4, nullptr, nullptr, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_autograsp(0, &ag, &grip, nullptr, 0, 4, nullptr, nullptr, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_autograsp(0, &ag, &grip, odd, 0, 4, nullptr, nullptr, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_autograsp(0, &ag, &grip, p, 0, 4, nullptr, nullptr, nullptr, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_autograsp(0, &ag, &by_share, p, 0, 4, nullptr, img, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_autograsp(0, &ag, &by_share, p, 0, 4, img, nullptr, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_autograsp(-1, &ag, &grip, p, 0, 4, nullptr, nullptr, img, pi, pi, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_sample_autograsp(0, &ag, &grip, p, 0, 4, nullptr, nullptr, img, pi, pi, nullptr) != VF_ERR_HIP) rc = 1;   // all through
                if (vf_cem_sample_autograsp(0, &ag, &by_share, p, 0, 4, img, img, img, pi, pi, nullptr) != VF_ERR_HIP) rc = 1;
                std::printf("  device CEM, autograsp: configuration and argument refusals: %s\n", rc ? "FAILED" : "ok");
                // the latent draws and their fold: plain arguments, no configuration
                struct { int n_latent, T, zdim; const char *msg; } bad_latents[] = {
                    {0, 3, 8, "n_latent"}, {2, 0, 8, "T = 0"}, {2, 3, 0, "zdim"}, {2, 1 << 20, 1 << 11, "2^30"}};
                for (const auto &c : bad_latents)
                    if (vf_cem_latents(0, 1u, 2u, 3u, c.n_latent, c.T, c.zdim, img, nullptr) != VF_ERR_INVALID ||
                        std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                        std::fprintf(stderr, "vf_cem_latents: want refusal '%s', got '%s'\n", c.msg, vf_last_error()); rc = 1;
                    }
                if (vf_cem_latents(0, 1u, 2u, 3u, 2, 3, 8, nullptr, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_latents(-1, 1u, 2u, 3u, 2, 3, 8, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_latents(0, 1u, 2u, 3u, 2, 3, 8, img, nullptr) != VF_ERR_HIP) rc = 1;           // all through: this build launches nothing
                struct { int M, n_latent, T, width, zdim; const char *msg; } bad_fold_latents[] = {
                    {0, 2, 3, 4, 8, "M = 0"}, {4, 0, 3, 4, 8, "n_latent"}, {4, 2, 0, 4, 8, "T = 0"}, {4, 2, 3, 0, 8, "width"},
                    {4, 2, 3, 4, 0, "zdim"}, {1 << 20, 1 << 11, 3, 4, 8, "rows do not fit"}, {4, 2, 1 << 28, 4, 4, "per row"}};
                for (const auto &c : bad_fold_latents)
                    if (vf_cem_fold_latents(0, img, img, c.M, c.n_latent, c.T, c.width, c.zdim, img, nullptr) != VF_ERR_INVALID ||
                        std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                        std::fprintf(stderr, "vf_cem_fold_latents: want refusal '%s', got '%s'\n", c.msg, vf_last_error()); rc = 1;
                    }
                if (vf_cem_fold_latents(0, nullptr, img, 4, 2, 3, 4, 8, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_fold_latents(0, img, img, 4, 2, 3, 4, 8, nullptr, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_fold_latents(-1, img, img, 4, 2, 3, 4, 8, img, nullptr) != VF_ERR_INVALID) rc = 1;
                if (vf_cem_fold_latents(0, img, img, 4, 2, 3, 4, 8, img, nullptr) != VF_ERR_HIP) rc = 1;
                std::printf("  device CEM, latent draws: argument refusals: %s\n", rc ? "FAILED" : "ok");
            }
            int32_t pix[2] = {0, 0};
            float out2[2];
            struct { vf_handle *h; int H, W; const float *cur; int ntask, region, clip; const char *msg; } reg[] = {
                {hh, 4, 64, img, 1, 0, 1, "H x W"},      {hh, 64, 7, img, 1, 0, 1, "H x W"},       {nullptr, 4, 4, img, 1, 0, 1, "H x W"},
                {hh, 4096, 4096, img, 1, 0, 1, "H x W"}, {nullptr, 64, 64, img, 1, 0, 1, "null argument"},
                {hh, 64, 64, nullptr, 1, 0, 1, "null argument"}, {hh, 64, 64, img, 0, 0, 1, "ntask"},
                {hh, 64, 64, img, 1, 6, 1, "region"},    {hh, 64, 64, img, 1, 0, 2, "clip_sub"}};
            for (const auto &c : reg) {
                const int r = vf_register_hw(c.h, c.H, c.W, c.cur, img, img, pix, c.ntask, c.region, c.clip, nullptr, nullptr, out2, out2, nullptr);
                if (r != VF_ERR_INVALID || std::string(vf_last_error()).find(c.msg) == std::string::npos) {
                    std::fprintf(stderr, "vf_register_hw: want refusal '%s', got rc %d '%s'\n", c.msg, r, vf_last_error()); rc = 1;
                }
            }
            std::printf("  area resampling / registration at the caller's size: refusals: %s\n", rc ? "FAILED" : "ok");
        }
        if (hh && vf_destroy(hh)) { std::fprintf(stderr, "vf_destroy after the injected failures failed\n"); rc = 1; }
        std::printf("  injected failures (bad_alloc, std::exception, foreign) in vf_create / vf_load_weights / build_schedule: %s\n",
                    rc ? "FAILED" : "status codes returned, handle reusable");
    }
    std::printf(rc ? "HOST SELFTEST FAILED\n" : "HOST SELFTEST OK\n");
    return rc;
}
