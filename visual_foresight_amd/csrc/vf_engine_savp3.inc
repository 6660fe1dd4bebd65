// vf_engine_savp3.inc - host side of arch 3, the published SAVP generator (textually included by vf_engine.hip behind the
// sinks): layer table, GEMM plans, buffers, weight re-packing and the emission of one rollout.
//
// Layer table and semantics: visual_foresight_amd/video_prediction/savp3_arch.py (the reference only instantiates the model
// class, visual_mpc/video_prediction/vpred_model_interface.py:52-58; its network lives in an absent package - parity unpinned).
// Device code: csrc/vf_savp3.h (element-wise items), vf_conv_mfma.h (EPI_RAW, gates_raw_epilogue).

namespace vf {

static const int kS3Ngf = 32;
static const float kS3Eps = 1e-6f;

struct S3Layer {                    // one encoder / decoder layer
    int idx = 0;
    bool dec = false, rnn = false;
    int k = 3;                      // conv kernel of the checkpoint (5 / 3)
    int cin = 0, C = 0;             // input channels (without the conditioning), output channels
    int hi = 0, wi = 0, ho = 0, wo = 0;
    int skip = -1;                  // decoder layer j > 0: the encoder layer whose output is concatenated
    int c_prev = 0, c_skip = 0;     // decoder: channels of the two up-sampled sources
    ConvLayer conv, lstm;           // GEMM plans: the conv (encoder: fused with its pool), the gate GEMM
    ConvLayer conv_pack;            // the conv as a plain layer (one 32-channel group per item): the plan its weights are packed
                                    // for; `conv` may run G = 2 / 4 of those groups per item on the same packed weights
    int cpi_n = 8, cpi_c = 8;       // channels per element-wise item (instance norm / cell)
    int up_rows = 0, up_items = 0;  // decoder: output rows per up-sampling item, items per sample
    // activations, [ncam * max_batch] samples each
    float *e = nullptr;             // conv output, normalised in place [ho * wo * C]
    float *u = nullptr;             // decoder: up-sampled concat input [ho * wo * cin]
    float *gates = nullptr, *c = nullptr, *hst[2] = {nullptr, nullptr};
    float *cb_conv = nullptr, *cb_lstm = nullptr;   // border-class biases [2 step parities][BV][25][C] / [..][25][4C]
};

struct S3ViewW {                    // device parameters of one view that are not packed GEMM weights
    float *ng[8] = {nullptr}, *nb[8] = {nullptr};           // instance norm of conv i
    float *lg[8] = {nullptr}, *lb[8] = {nullptr};           // gate norm of conv-LSTM i [4C]
    float *cg[8] = {nullptr}, *cb[8] = {nullptr};           // cell-state norm [C]
    float *wc_conv[8] = {nullptr}, *wc_lstm[8] = {nullptr}; // conditioning rows [taps][ncond][Ctot]
    float *hmhs_g = nullptr, *hmhs_b = nullptr;             // instance norm of the two heads' hidden layers, [hm 32 | hs 32]
    float *w_rnnz = nullptr, *b_rnnz = nullptr;
    // the heads' output convs in the layout the fused second phase (EW_TOP3) reads: [9][32][4] / [9][kT3MaskIn][8]
    float *w_scr_v = nullptr, *b_scr_v = nullptr, *w_msk_v = nullptr, *b_msk_v = nullptr;
};

struct Savp3 {
    int n_enc = 0, n_dec = 0, nl = 0;
    int a_env = 0, ncond = 0, zdim = 0;
    S3Layer L[8];
    // the hidden layers of the mask and scratch heads read the same tensor: ONE conv item with two 32-channel "gates" (hmhs;
    // hmhs_pack = the same layer seen as one 64-channel conv, whose packed weights it shares)
    ConvLayer hmhs, hmhs_pack, scratch, masks;
    std::vector<S3ViewW> vw;
    // heads, [ncam * max_batch] samples
    float *hmhs_raw = nullptr, *hm_o = nullptr, *hs_o = nullptr, *scr_raw = nullptr, *trans = nullptr, *transd = nullptr, *mlog = nullptr;
    float *norm_tab = nullptr;      // [BV][64][2]: instance-norm (scale, shift) of the heads' hidden layers (EW_TOP3)
    float *condvec = nullptr;       // [S][BV][ncond]
    float *rnn_state = nullptr;     // [BV][2 zdim]
    int top_tiles = 0;
};

static void s3_specs(int H, int W, int layer_spec, std::vector<std::pair<int, bool>> &enc, std::vector<std::pair<int, bool>> &dec) {
    const int scale = layer_spec ? layer_spec : std::min(H, W), n = kS3Ngf;
    if (scale >= 128) {
        enc = {{n, false}, {2 * n, true}, {4 * n, true}, {8 * n, true}};
        dec = {{8 * n, true}, {4 * n, true}, {2 * n, true}, {n, false}};
    } else if (scale >= 64) {
        enc = {{n, true}, {2 * n, true}, {4 * n, true}};
        dec = {{2 * n, true}, {n, true}, {n / 2, false}};
    } else {
        enc = {{n, true}, {2 * n, true}};
        dec = {{n, true}, {n / 2, false}};
    }
}

// geometry of every layer (no plans): shared by the tensor table, the MAC count and s3_create
static int s3_layer_table(const vf_config &c, S3Layer (&L)[8], int &n_enc, int &n_dec) {
    std::vector<std::pair<int, bool>> enc, dec;
    s3_specs(c.height, c.width, c.layer_spec, enc, dec);
    n_enc = (int)enc.size(); n_dec = (int)dec.size();
    int cin = 6, h = c.height, w = c.width;
    for (int i = 0; i < n_enc; ++i) {
        S3Layer &l = L[i];
        l.idx = i; l.dec = false; l.rnn = enc[i].second; l.k = i == 0 ? 5 : 3; l.cin = cin; l.C = enc[i].first;
        l.hi = h; l.wi = w; l.ho = h / 2; l.wo = w / 2; l.skip = -1;
        h /= 2; w /= 2; cin = l.C;
    }
    for (int j = 0; j < n_dec; ++j) {
        S3Layer &l = L[n_enc + j];
        l.idx = n_enc + j; l.dec = true; l.rnn = dec[j].second; l.k = 3; l.C = dec[j].first;
        l.c_prev = cin; l.skip = j > 0 ? n_enc - j - 1 : -1; l.c_skip = l.skip >= 0 ? L[l.skip].C : 0;
        l.cin = l.c_prev + l.c_skip;
        l.hi = h; l.wi = w; l.ho = 2 * h; l.wo = 2 * w;
        h *= 2; w *= 2; cin = l.C;
    }
    return n_enc + n_dec;
}

static std::vector<TensorDesc> s3_tensor_table(const vf_config &c) {
    std::vector<TensorDesc> t;
    size_t off = 0;
    auto add = [&](const std::string &name, std::vector<int> shape) {
        TensorDesc d;
        d.name = name; d.rank = (int)shape.size();
        for (int i = 0; i < 4; ++i) d.shape[i] = i < d.rank ? shape[i] : 1;
        d.offset = off; off += d.size();
        t.push_back(d);
    };
    S3Layer L[8];
    int n_enc, n_dec;
    const int nl = s3_layer_table(c, L, n_enc, n_dec);
    const int a_env = c.adim - c.zdim, nc = a_env + c.sdim + c.zdim;
    for (int i = 0; i < nl; ++i) {
        const std::string n = "h" + std::to_string(i);
        add(n + "c/w", {L[i].k, L[i].k, L[i].cin + nc, L[i].C}); add(n + "c/b", {L[i].C});
        add(n + "n/g", {L[i].C}); add(n + "n/b", {L[i].C});
        if (L[i].rnn) {
            add(n + "l/w", {5, 5, 2 * L[i].C + nc, 4 * L[i].C});
            add(n + "lg/g", {4 * L[i].C}); add(n + "lg/b", {4 * L[i].C});
            add(n + "lc/g", {L[i].C}); add(n + "lc/b", {L[i].C});
        }
    }
    const int top = L[nl - 1].C;
    for (const char *n : {"hm", "hs"}) {
        add(std::string(n) + "/w", {3, 3, top, kS3Ngf}); add(std::string(n) + "/b", {kS3Ngf});
        add(std::string(n) + "n/g", {kS3Ngf}); add(std::string(n) + "n/b", {kS3Ngf});
    }
    add("scratch/w", {3, 3, kS3Ngf, 3}); add("scratch/b", {3});
    add("masks/w", {3, 3, kS3Ngf + 3 * (kNumWarp3 + 3), kNumWarp3 + 3}); add("masks/b", {kNumWarp3 + 3});
    const S3Layer &bot = L[n_enc - 1];
    add("cdna/w", {bot.ho * bot.wo * bot.C, kTaps * kNumWarp3}); add("cdna/b", {kTaps * kNumWarp3});
    add("state/w", {a_env + c.sdim, c.sdim}); add("state/b", {c.sdim});
    add("rnnz/w", {2 * c.zdim, 4 * c.zdim}); add("rnnz/b", {4 * c.zdim});
    return t;
}

// algorithmic MACs per sample-step as the checkpoint describes the network (savp3_arch.py, macs_per_sample_step)
static double s3_macs(const vf_config &c) {
    S3Layer L[8];
    int n_enc, n_dec;
    const int nl = s3_layer_table(c, L, n_enc, n_dec);
    const double nc = (c.adim - c.zdim) + c.sdim + c.zdim, H = c.height, W = c.width;
    double m = 0;
    for (int i = 0; i < nl; ++i) {
        const S3Layer &l = L[i];
        const double r = l.dec ? (double)l.ho * l.wo : (double)l.hi * l.wi;
        m += r * l.k * l.k * (l.cin + nc) * l.C;
        if (l.rnn) m += (double)l.ho * l.wo * 25.0 * (2 * l.C + nc) * 4 * l.C;
    }
    const double top = L[nl - 1].C;
    m += 2 * H * W * 9 * top * kS3Ngf + H * W * 9 * kS3Ngf * 3 + H * W * 9 * (kS3Ngf + 3 * (kNumWarp3 + 3)) * (kNumWarp3 + 3);
    const S3Layer &bot = L[n_enc - 1];
    m += (double)bot.ho * bot.wo * bot.C * kTaps * kNumWarp3;
    m += H * W * kTaps * (3 + c.ndesig) * kNumWarp3;
    m += ((c.adim - c.zdim) + c.sdim) * (double)c.sdim + 2.0 * c.zdim * 4 * c.zdim;
    return m;
}

static int s3_validate(const vf_config *c) {
    if (c->num_masks != kNumWarp3) return fail(VF_ERR_INVALID, "arch 3 composes four CDNA warps: num_masks must be 4");
    if (c->precision != 0) return fail(VF_ERR_INVALID, "arch 3 is built for precision 0 (exact fp32) only");
    if (c->zdim < 1 || c->zdim >= c->adim || c->zdim > 16)
        return fail(VF_ERR_INVALID, "arch 3: adim includes the zdim latent channels (1 <= zdim < adim, zdim <= 16)");
    if (c->layer_spec != 0 && c->layer_spec != 32 && c->layer_spec != 64 && c->layer_spec != 128)
        return fail(VF_ERR_INVALID, "arch 3: layer_spec must be 0 (by image size), 32, 64 or 128");
    const int scale = c->layer_spec ? c->layer_spec : std::min(c->height, c->width);
    if (scale < 32) return fail(VF_ERR_INVALID, "arch 3 needs images of at least 32 x 32");
    const int f = scale >= 128 ? 16 : (scale >= 64 ? 8 : 4);
    if (c->height % f || c->width % f || c->height / f < 4 || c->width / f < 4)
        return fail(VF_ERR_INVALID, "arch 3: height/width must be multiples of " + std::to_string(f) + " and at least " +
                                        std::to_string(4 * f));
    return VF_OK;
}

// Channels per element-wise item.  An item owns ALL pixels of its channel group, and a pixel's channels are contiguous in
// memory: 32 channels = one 128-byte line per (pixel, gate) - a narrower group (the first version took 4 - 8 channels to keep
// items short) fetches the same lines for a fraction of their bytes: at the C5 shard the items ran 71 us each ALONE on their
// CU (tools/trace_cu.py) for a few KB of useful data per thread.  Fewer, longer items; the batch supplies the parallelism.
static int s3_cpi(int HW, int C) {
    (void)HW;
    int cpi = 32;
#ifdef VF_DEBUG_KNOBS
    if (const char *e = getenv("VF_S3_CPI")) cpi = std::max(4, std::min(32, atoi(e)));
#endif
    while (cpi > C) cpi >>= 1;
    return std::max(cpi, 4);
}

// 256-row tiles (two MFMA row blocks per wave: every weight load feeds two blocks) for every conv whose image supplies the rows
static int s3_rows(int ho, int wo, int C) {
    (void)C;
    return ho * wo >= 256 ? 256 : 128;
}

static int s3_create(vf_handle *h) {
    const vf_config &c = h->cfg;
    Savp3 *s = new Savp3();
    h->s3 = s;
    s->nl = s3_layer_table(c, s->L, s->n_enc, s->n_dec);
    s->a_env = c.adim - c.zdim; s->zdim = c.zdim; s->ncond = s->a_env + c.sdim + c.zdim;
    const int H = h->H, W = h->W, ND = h->ND, NV = h->ncam;
    const size_t BV = (size_t)c.max_batch * NV;
    int rc;
    h->layers.clear();
    for (int i = 0; i < s->nl; ++i) {
        S3Layer &l = s->L[i];
        const std::string nm = "h" + std::to_string(i) + "c";
        // Layers with few channels at 64 x 64 pixels and more (the first encoder conv, the last decoder conv, the heads) are
        // dominated by per-item overhead - a 128-row item is ~4 us of MFMAs in 11 - 27 us: they take 256-row tiles (two row
        // blocks per wave, conv_tile<.., EPI_RAW, 2>): half the items, the same arithmetic per output
        const int rows = s3_rows(l.ho, l.wo, l.C);
        if (!l.dec) {
            // conv k x k / 1 + 2x2 average pool = ONE (k + 1) x (k + 1) / 2 convolution with the box-filtered kernel
            // (its stride-2 input tile is four times the output tile: the 256-row plan only where it keeps the chunk size)
            const int p = (l.k - 1) / 2;
            auto plan = [&](const int r) {
                if (i == 0) init_layer(l.conv, nm.c_str(), PACK_PLAIN, l.hi, l.wi, l.ho, l.wo, l.k + 1, l.k + 1, 2, p, 3, 3, l.C, false, false, r);
                else init_layer(l.conv, nm.c_str(), PACK_PLAIN, l.hi, l.wi, l.ho, l.wo, l.k + 1, l.k + 1, 2, p, l.cin, 0, l.C, false, false, r);
            };
            plan(128);
            const int kc1 = l.conv.KC;
            if (rows == 256) { plan(256); if (l.conv.KC != kc1) plan(128); }
        } else {
            init_layer(l.conv, nm.c_str(), PACK_PLAIN, l.ho, l.wo, l.ho, l.wo, 3, 3, 1, 1, l.cin, 0, l.C, false, false, rows);
            const int cq = l.cin / 4;
            l.up_rows = std::max(1, std::min(l.ho, 24576 / (l.wo * cq)));
            l.up_items = (l.ho + l.up_rows - 1) / l.up_rows;
        }
        // Convs of 64 / 128 / 256 channels: two / four 32-channel groups per item (conv_tile<G, EPI_RAW>; the groups are the
        // item's "gates", the packed weights stay those of the plain layer) - the haloed input tile, whose staging is what a
        // 3 x 3 layer spends its time on (9 taps per staged chunk), is staged once for 64 / 128 output channels
        l.conv_pack = l.conv;
        {
            int G = l.C % 128 == 0 ? 4 : (l.C % 64 == 0 ? 2 : 1);
#ifdef VF_DEBUG_KNOBS
            if (const char *e = getenv("VF_S3_CONV_G")) G = std::min(G, std::max(1, atoi(e)));
#endif
            if (G == 4 && l.conv.mrep != 1) {       // four accumulator tiles per row block: 128-row items
                if (!l.dec) {
                    const int p = (l.k - 1) / 2;
                    init_layer(l.conv, nm.c_str(), PACK_PLAIN, l.hi, l.wi, l.ho, l.wo, l.k + 1, l.k + 1, 2, p, l.cin, 0, l.C, false, false, 128);
                } else {
                    init_layer(l.conv, nm.c_str(), PACK_PLAIN, l.ho, l.wo, l.ho, l.wo, 3, 3, 1, 1, l.cin, 0, l.C, false, false, 128);
                }
                if (l.conv.KC != l.conv_pack.KC) l.conv = l.conv_pack, G = 2;      // (keep the packed chunking)
                else l.conv_pack = l.conv;
            }
            const int steps = l.conv.KH * l.conv.KW * (l.conv.KC / 8);      // K steps per chunk: whole weight rings (conv_tile)
            if (G == 4 && steps % 4) G = 2;
            if (G == 2 && steps % 2) G = 1;
            if (i == 0) G = 1;                      // (the first conv reads two 3-channel segments: plain)
            if (G > 1) { l.conv.G = G; l.conv.ncg = l.C / (32 * G); l.conv.Cout = l.C / G; l.conv.n_valid = l.C / G; }
        }
        h->layers.push_back(&l.conv);
        l.cpi_n = s3_cpi(l.ho * l.wo, l.C);
        if (l.rnn) {
            const std::string ln = "h" + std::to_string(i) + "l";
            init_layer(l.lstm, ln.c_str(), PACK_LSTM, l.ho, l.wo, l.ho, l.wo, 5, 5, 1, 2, l.C, l.C, l.C, true, false, 128, 0,
                       false, s->ncond);
            if (l.lstm.tile != TILE_LSTM_GS128 || l.lstm.KC != 32)
                return fail(VF_ERR_INVALID, "arch 3: conv-LSTM " + ln + " does not fit the gate-split tile");
            h->layers.push_back(&l.lstm);
            l.cpi_c = s3_cpi(l.ho * l.wo, l.C);
        }
        if (l.cin % 4 && i > 0) return fail(VF_ERR_INVALID, "arch 3: channel counts must be multiples of 4");
    }
    const int top = s->L[s->nl - 1].C;
    const int rows_top = s3_rows(H, W, kS3Ngf);
    init_layer(s->hmhs_pack, "hmhs", PACK_PLAIN, H, W, H, W, 3, 3, 1, 1, top, 0, 2 * kS3Ngf, false, false, rows_top);
    s->hmhs = s->hmhs_pack;
    s->hmhs.G = 2; s->hmhs.ncg = 1; s->hmhs.Cout = kS3Ngf; s->hmhs.n_valid = kS3Ngf;
    if ((s->hmhs.KH * s->hmhs.KW * (s->hmhs.KC / 8)) % 2)
        return fail(VF_ERR_INVALID, "arch 3: the fused head conv needs an even number of K steps per chunk");
    init_layer(s->scratch, "scratch", PACK_PLAIN, H, W, H, W, 3, 3, 1, 1, kS3Ngf, 0, kScrCh, false, false, rows_top);
    init_layer(s->masks, "masks", PACK_PLAIN, H, W, H, W, 3, 3, 1, 1, kS3Ngf, kTransCh, kMaskCh, false, false, rows_top);
    for (ConvLayer *l : {&s->hmhs, &s->scratch, &s->masks}) h->layers.push_back(l);
    const S3Layer &bot = s->L[s->n_enc - 1];
    plan_fc(h, bot.ho * bot.wo * bot.C, h->K);
    h->layers.push_back(&h->fc);
    if ((int)h->layers.size() > kNumConvLayers) return fail(VF_ERR_INVALID, "arch 3: too many GEMM layers");
    h->max_lds = ew_lds_bytes(EW_TOP3, h->ND);
    for (size_t i = 0; i < h->layers.size(); ++i) {
        h->layers[i]->id = (int)i;
        h->max_lds = std::max(h->max_lds, h->layers[i]->lds_bytes);
    }
    h->fc_wide.id = h->fc.id;
    s->hmhs_pack.id = s->hmhs.id;
    for (int i = 0; i < s->nl; ++i) s->L[i].conv_pack.id = s->L[i].conv.id;
    h->max_lds = std::max(h->max_lds, h->fc_wide.lds_bytes) + 16;
    h->dedup = false;               // every sample runs every step (no context de-duplication in arch 3)
    h->small_plans = false;
    s->top_tiles = h->ntiles;

#define S3_ALLOC(ptr, n)                           \
    do {                                           \
        rc = dev_alloc(h, &(ptr), (size_t)(n));    \
        if (rc) return rc;                         \
    } while (0)
    const int ncond = s->ncond;
    h->views.resize(NV);
    s->vw.resize(NV);
    for (int v = 0; v < NV; ++v) {
        ViewData &vd = h->views[v];
        S3ViewW &w = s->vw[v];
        for (const ConvLayer *l : h->layers) {
            S3_ALLOC(vd.lw[l->id].w, l->packed_w());
            S3_ALLOC(vd.lw[l->id].b, l->packed_b());
        }
        for (int i = 0; i < s->nl; ++i) {
            const S3Layer &l = s->L[i];
            S3_ALLOC(w.ng[i], l.C); S3_ALLOC(w.nb[i], l.C);
            S3_ALLOC(w.wc_conv[i], (size_t)l.conv.KH * l.conv.KW * ncond * l.C);
            if (l.rnn) {
                S3_ALLOC(w.lg[i], 4 * l.C); S3_ALLOC(w.lb[i], 4 * l.C);
                S3_ALLOC(w.cg[i], l.C); S3_ALLOC(w.cb[i], l.C);
                S3_ALLOC(w.wc_lstm[i], (size_t)25 * ncond * 4 * l.C);
            }
        }
        S3_ALLOC(w.hmhs_g, 2 * kS3Ngf); S3_ALLOC(w.hmhs_b, 2 * kS3Ngf);
        S3_ALLOC(w.w_rnnz, (size_t)2 * c.zdim * 4 * c.zdim); S3_ALLOC(w.b_rnnz, 4 * c.zdim);
        S3_ALLOC(w.w_scr_v, 9 * kS3Ngf * 4); S3_ALLOC(w.b_scr_v, 4);
        S3_ALLOC(w.w_msk_v, 9 * kT3MaskIn * 8); S3_ALLOC(w.b_msk_v, 8);
        S3_ALLOC(vd.w_state, (size_t)(s->a_env + c.sdim) * c.sdim); S3_ALLOC(vd.b_state, c.sdim);
        S3_ALLOC(vd.b_fc, kTaps * h->K);
    }
    for (int i = 0; i < s->nl; ++i) {
        S3Layer &l = s->L[i];
        const size_t px = (size_t)l.ho * l.wo;
        S3_ALLOC(l.e, BV * px * l.C);
        if (l.dec) S3_ALLOC(l.u, BV * px * l.cin);
        S3_ALLOC(l.cb_conv, 2 * BV * 25 * l.C);
        if (l.rnn) {
            S3_ALLOC(l.gates, BV * px * 4 * l.C);
            S3_ALLOC(l.c, BV * px * l.C);
            S3_ALLOC(l.hst[0], BV * px * l.C);
            S3_ALLOC(l.hst[1], BV * px * l.C);
            S3_ALLOC(l.cb_lstm, 2 * BV * 25 * 4 * l.C);
        }
    }
    const size_t HW = (size_t)H * W;
    S3_ALLOC(s->hmhs_raw, BV * HW * 2 * kS3Ngf);
    S3_ALLOC(s->hm_o, BV * HW * kS3Ngf);
    S3_ALLOC(s->hs_o, BV * HW * kS3Ngf);
    S3_ALLOC(s->scr_raw, BV * HW * kScrCh);
    S3_ALLOC(s->trans, BV * HW * kTransCh);
    S3_ALLOC(s->transd, BV * HW * kNumWarp3 * ND);
    S3_ALLOC(s->mlog, BV * HW * kMaskCh);
    S3_ALLOC(s->norm_tab, BV * 128);
    S3_ALLOC(s->condvec, (size_t)h->S * BV * ncond);
    S3_ALLOC(s->rnn_state, BV * 2 * c.zdim);
#undef S3_ALLOC
    // (of the rows of a BatchView an arch 3 engine has the CDNA kernels' and the predictions': its layers' buffers are above)
    row_spec(h, h->base.fc_part, (size_t)h->fc.nsplit * kTaps * h->K, false);
    row_spec(h, h->base.kern, (size_t)kTaps * h->K, false);
    h->shared_views.resize(NV);         // (all null: no context de-duplication)
    return alloc_common(h, 80);
}

static void s3_free(vf_handle *h) {
    delete h->s3;
    h->s3 = nullptr;
}

// border-class coefficient tables f[class][tap] (vf_savp3.h)
static void s3_ftab_lstm(float (&f)[5][8]) {
    memset(f, 0, sizeof(f));
    for (int r = 0; r < 5; ++r)
        for (int t = 0; t < 5; ++t) f[r][t] = (t >= cond_tap_lo(r) && t < cond_tap_hi(r)) ? 1.f : 0.f;
}
static void s3_ftab_pool(float (&f)[5][8], int k) {     // fused (k + 1)^2 / 2 conv, pad (k - 1) / 2
    memset(f, 0, sizeof(f));
    const int K = k + 1, p = (k - 1) / 2;
    for (int r = 0; r < 5; ++r)
        for (int t = 0; t < K; ++t) f[r][t] = r == 0 ? (t >= p ? 1.f : 0.f) : (r == 4 ? (t < p + 2 ? 1.f : 0.f) : 1.f);
}
static void s3_ftab_up(float (&f)[5][8]) {              // 3x3 conv over the bilinearly up-sampled constant
    memset(f, 0, sizeof(f));
    const float tab[5][3] = {{0.f, .75f, 1.f}, {.75f, 1.f, 1.f}, {1.f, 1.f, 1.f}, {1.f, 1.f, .75f}, {1.f, .75f, 0.f}};
    for (int r = 0; r < 5; ++r)
        for (int t = 0; t < 3; ++t) f[r][t] = tab[r][t];
}

// canonical [k][k][Cin][C] -> [(k+1)][(k+1)][Cin][C]: the kernel of "conv k x k, then 2 x 2 average pool" as one stride-2 conv
static std::vector<float> s3_box_filter(const float *w, int k, int Cin, int C) {
    const int K = k + 1;
    std::vector<float> out((size_t)K * K * Cin * C);
    for (int u = 0; u < K; ++u)
        for (int v = 0; v < K; ++v)
            for (size_t i = 0; i < (size_t)Cin * C; ++i) {
                double a = 0.0;
                for (int da = 0; da < 2; ++da)
                    for (int db = 0; db < 2; ++db) {
                        const int y = u - da, x = v - db;
                        if (y >= 0 && y < k && x >= 0 && x < k) a += (double)w[((size_t)y * k + x) * Cin * C + i];
                    }
                out[((size_t)u * K + v) * Cin * C + i] = (float)(0.25 * a);
            }
    return out;
}

static int s3_load_weights(vf_handle *h, const float *blob, int view) {
    Savp3 *s = h->s3;
    ViewData &vd = h->views[view];
    S3ViewW &vw = s->vw[view];
    const int ncond = s->ncond;
    int rc;
    auto T = [&](const std::string &name) { return find_tensor(h->table, name); };
    auto put = [&](float *dst, const std::string &name) {
        const TensorDesc *d = T(name);
        return dev_write(h, dst, blob + d->offset, d->size() * sizeof(float));
    };
    auto put_layer = [&](const ConvLayer &l, const std::vector<float> &wp, const std::vector<float> &bp) -> int {
        if (wp.size() != l.packed_w() || bp.size() != l.packed_b())
            return fail(VF_ERR_INVALID, "internal: packed size of " + l.name + " differs from its plan");
        int r;
        if ((r = dev_write(h, vd.lw[l.id].w, wp.data(), wp.size() * sizeof(float)))) return r;
        return dev_write(h, vd.lw[l.id].b, bp.data(), bp.size() * sizeof(float));
    };
    for (int i = 0; i < s->nl; ++i) {
        const S3Layer &l = s->L[i];
        const std::string n = "h" + std::to_string(i);
        const TensorDesc *w = T(n + "c/w"), *b = T(n + "c/b");
        const int Cin = w->shape[2], C = w->shape[3];
        // real input channels / conditioning rows of the canonical kernel
        std::vector<float> wr((size_t)l.k * l.k * l.cin * C), wc((size_t)l.k * l.k * ncond * C);
        for (int tap = 0; tap < l.k * l.k; ++tap) {
            memcpy(&wr[(size_t)tap * l.cin * C], blob + w->offset + (size_t)tap * Cin * C, (size_t)l.cin * C * sizeof(float));
            memcpy(&wc[(size_t)tap * ncond * C], blob + w->offset + ((size_t)tap * Cin + l.cin) * C, (size_t)ncond * C * sizeof(float));
        }
        if (!l.dec) {
            wr = s3_box_filter(wr.data(), l.k, l.cin, C);
            wc = s3_box_filter(wc.data(), l.k, ncond, C);
        }
        if ((rc = put_layer(l.conv_pack, pack_weights(l.conv_pack, wr.data(), l.conv.KH, l.conv.KW, l.cin, C), pack_bias(l.conv_pack, blob + b->offset)))) return rc;
        if ((rc = dev_write(h, vw.wc_conv[i], wc.data(), wc.size() * sizeof(float)))) return rc;
        if ((rc = put(vw.ng[i], n + "n/g")) || (rc = put(vw.nb[i], n + "n/b"))) return rc;
        if (!l.rnn) continue;
        const TensorDesc *lw = T(n + "l/w");
        const int LCin = lw->shape[2], C4 = lw->shape[3];
        std::vector<float> zero_b((size_t)C4, 0.f);
        if ((rc = put_layer(l.lstm, pack_weights(l.lstm, blob + lw->offset, 5, 5, LCin, C4), pack_bias(l.lstm, zero_b.data())))) return rc;
        std::vector<float> lc((size_t)25 * ncond * C4);
        for (int tap = 0; tap < 25; ++tap)
            memcpy(&lc[(size_t)tap * ncond * C4], blob + lw->offset + ((size_t)tap * LCin + l.C) * C4, (size_t)ncond * C4 * sizeof(float));
        if ((rc = dev_write(h, vw.wc_lstm[i], lc.data(), lc.size() * sizeof(float)))) return rc;
        if ((rc = put(vw.lg[i], n + "lg/g")) || (rc = put(vw.lb[i], n + "lg/b")) || (rc = put(vw.cg[i], n + "lc/g")) ||
            (rc = put(vw.cb[i], n + "lc/b")))
            return rc;
    }
    {   // hm | hs -> one conv with 64 output channels (column = gate * 32 + channel: the layout of the two-gate item)
        const TensorDesc *wm = T("hm/w"), *ws = T("hs/w"), *bm = T("hm/b"), *bs = T("hs/b");
        const int Cin = wm->shape[2];
        std::vector<float> wp((size_t)9 * Cin * 2 * kS3Ngf), bp(2 * kS3Ngf);
        for (int r = 0; r < 9 * Cin; ++r)
            for (int o = 0; o < kS3Ngf; ++o) {
                wp[(size_t)r * 2 * kS3Ngf + o] = (blob + wm->offset)[(size_t)r * kS3Ngf + o];
                wp[(size_t)r * 2 * kS3Ngf + kS3Ngf + o] = (blob + ws->offset)[(size_t)r * kS3Ngf + o];
            }
        for (int o = 0; o < kS3Ngf; ++o) { bp[o] = (blob + bm->offset)[o]; bp[kS3Ngf + o] = (blob + bs->offset)[o]; }
        if ((rc = put_layer(s->hmhs_pack, pack_weights(s->hmhs_pack, wp.data(), 3, 3, Cin, 2 * kS3Ngf), pack_bias(s->hmhs_pack, bp.data())))) return rc;
    }
    if ((rc = put(vw.hmhs_g, "hmn/g")) || (rc = put(vw.hmhs_g + kS3Ngf, "hsn/g")) || (rc = put(vw.hmhs_b, "hmn/b")) ||
        (rc = put(vw.hmhs_b + kS3Ngf, "hsn/b")))
        return rc;
    {   // scratch head: 3 -> kScrCh output channels (zero weights in the pad)
        const TensorDesc *w = T("scratch/w"), *b = T("scratch/b");
        std::vector<float> wp((size_t)9 * kS3Ngf * kScrCh, 0.f), bp(kScrCh, 0.f);
        for (int r = 0; r < 9 * kS3Ngf; ++r)
            for (int o = 0; o < 3; ++o) wp[(size_t)r * kScrCh + o] = (blob + w->offset)[(size_t)r * 3 + o];
        for (int o = 0; o < 3; ++o) bp[o] = (blob + b->offset)[o];
        if ((rc = put_layer(s->scratch, pack_weights(s->scratch, wp.data(), 3, 3, kS3Ngf, kScrCh), pack_bias(s->scratch, bp.data())))) return rc;
    }
    {   // mask head: [h_masks 32 | 21 layer channels] -> [32 | kTransCh], 7 -> kMaskCh outputs
        const TensorDesc *w = T("masks/w"), *b = T("masks/b");
        const int Cin = w->shape[2], NM = w->shape[3], CinP = kS3Ngf + kTransCh;
        std::vector<float> wp((size_t)9 * CinP * kMaskCh, 0.f), bp(kMaskCh, 0.f);
        for (int tap = 0; tap < 9; ++tap)
            for (int ci = 0; ci < Cin; ++ci)
                for (int o = 0; o < NM; ++o)
                    wp[((size_t)tap * CinP + ci) * kMaskCh + o] = (blob + w->offset)[((size_t)tap * Cin + ci) * NM + o];
        for (int o = 0; o < NM; ++o) bp[o] = (blob + b->offset)[o];
        if ((rc = put_layer(s->masks, pack_weights(s->masks, wp.data(), 3, 3, CinP, kMaskCh), pack_bias(s->masks, bp.data())))) return rc;
    }
    {   // the same two output convs for the fused second phase (EW_TOP3): VALU layouts, weights as scalar operands
        const TensorDesc *w = T("scratch/w"), *b = T("scratch/b");
        std::vector<float> ws((size_t)9 * kS3Ngf * 4, 0.f), bs(4, 0.f);
        for (int r = 0; r < 9 * kS3Ngf; ++r)
            for (int o = 0; o < 3; ++o) ws[(size_t)r * 4 + o] = (blob + w->offset)[(size_t)r * 3 + o];
        for (int o = 0; o < 3; ++o) bs[o] = (blob + b->offset)[o];
        if ((rc = dev_write(h, vw.w_scr_v, ws.data(), ws.size() * sizeof(float))) || (rc = dev_write(h, vw.b_scr_v, bs.data(), 16))) return rc;
        const TensorDesc *mw = T("masks/w"), *mb = T("masks/b");
        const int Cin = mw->shape[2], NM = mw->shape[3];
        std::vector<float> wm((size_t)9 * kT3MaskIn * 8, 0.f), bm(8, 0.f);
        for (int tap = 0; tap < 9; ++tap)
            for (int ci = 0; ci < Cin; ++ci)
                for (int o = 0; o < NM; ++o)
                    wm[((size_t)tap * kT3MaskIn + ci) * 8 + o] = (blob + mw->offset)[((size_t)tap * Cin + ci) * NM + o];
        for (int o = 0; o < NM; ++o) bm[o] = (blob + mb->offset)[o];
        if ((rc = dev_write(h, vw.w_msk_v, wm.data(), wm.size() * sizeof(float))) || (rc = dev_write(h, vw.b_msk_v, bm.data(), 32))) return rc;
    }
    {
        const TensorDesc *w = T("cdna/w");
        std::vector<float> zb(h->fc.packed_b(), 0.f);
        if ((rc = put_layer(h->fc, pack_weights(h->fc, blob + w->offset, 1, 1, w->shape[0], w->shape[1]), zb))) return rc;
    }
    if ((rc = put(vd.b_fc, "cdna/b")) || (rc = put(vd.w_state, "state/w")) || (rc = put(vd.b_state, "state/b")) ||
        (rc = put(vw.w_rnnz, "rnnz/w")) || (rc = put(vw.b_rnnz, "rnnz/b")))
        return rc;
    return VF_OK;
}

// ------------------------------------------------------------------ one rollout of one view
template <class Sink>
static int emit_rollout_s3(vf_handle *h, int view, int B, const float *d_actions, const int32_t *goal_pix, Sink &sink) {
    const vf_config &c = h->cfg;
    Savp3 *s = h->s3;
    const ViewData &vd = h->views[view];
    const S3ViewW &vw = s->vw[view];
    const int H = h->H, W = h->W, ND = h->ND, nc = c.n_context, ncond = s->ncond;
    const size_t BV = (size_t)c.max_batch * h->ncam;
    const size_t row = (size_t)view * c.max_batch;         // first row of this view in every [ncam][max_batch] buffer
    const long long HW = (long long)H * W;
    const BatchView bv = make_view(h, view, d_actions);

    auto params = [&](const ConvLayer &l, const SegArg &s0, const SegArg *s1) { return make_params(l, vd.lw[l.id], B, s0, s1, h->pad_skip); };
    auto ew_base = [&](int op, int gx, int spi) {
        EwParams e; memset(&e, 0, sizeof(e)); e.op = op; e.B = B; e.gx = gx; e.spi = spi; return e;
    };

    int last = -1, last2 = -1;          // terminal unit of the previous step / of the one before
    int u_sa_prev = -1;
    int u_cell_prev[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    int u_cc_all[2][8], u_cl_all[2][8];     // [step parity]: the class-bias units of that step
    // State FC, rnn_z, the conditioning vector of step `sx` and the border-class biases it gives every conv and conv-LSTM.
    // Nothing here depends on the images: the chain SA3(0) -> SA3(1) -> ... runs ahead, and the tables of step sx (two
    // buffers by step parity) are computed while step sx - 1 is still rolling - `guard` = the terminal unit of step sx - 2,
    // whose element-wise items were the last readers of that parity's tables.
    auto emit_cond = [&](const int sx, const int guard) -> int {
        const int par = sx & 1;
        const StepIo ic = step_io(h, view, bv, sx);
        EwParams e = ew_base(EW_SA3, 0, kSaPerItem);
        e.sa.action = ic.action; e.sa.action_bs = ic.action_bs; e.sa.state = ic.state; e.sa.state_bs = ic.state_bs;
        e.sa.adim = c.adim; e.sa.sdim = c.sdim; e.sa.zdim = c.zdim;
        e.sa.w_state = vd.w_state; e.sa.b_state = vd.b_state; e.sa.w_rnnz = vw.w_rnnz; e.sa.b_rnnz = vw.b_rnnz;
        e.sa.rnn_state = s->rnn_state + row * 2 * c.zdim; e.sa.first = sx == 0;
        float *condvec = s->condvec + ((size_t)sx * BV + row) * ncond;
        e.sa.condvec = condvec;
        e.sa.state_out = ic.state_out; e.sa.state_out_bs = ic.state_out_bs;
        VF_EMIT(u_sa, sink.ew(e, view, {u_sa_prev}))
        u_sa_prev = u_sa;
        for (int i = 0; i < s->nl; ++i) {
            const S3Layer &l = s->L[i];
            EwParams q = ew_base(EW_COND3, 0, kCond3PerItem);
            q.cond.condvec = condvec; q.cond.ncond = ncond; q.cond.w = vw.wc_conv[i]; q.cond.Ctot = l.C; q.cond.KH = l.conv.KH;
            if (l.dec) s3_ftab_up(q.cond.f); else s3_ftab_pool(q.cond.f, l.k);
            q.cond.out = l.cb_conv + ((size_t)par * BV + row) * 25 * l.C;
            VF_EMIT(ucc, sink.ew(q, view, {u_sa, guard}))
            u_cc_all[par][i] = ucc; u_cl_all[par][i] = -1;
            if (!l.rnn) continue;
            q.cond.w = vw.wc_lstm[i]; q.cond.Ctot = 4 * l.C; q.cond.KH = 5;
            s3_ftab_lstm(q.cond.f);
            q.cond.out = l.cb_lstm + ((size_t)par * BV + row) * 25 * 4 * l.C;
            VF_EMIT(ucl, sink.ew(q, view, {u_sa, guard}))
            u_cl_all[par][i] = ucl;
        }
        return VF_OK;
    };
    {
        const int rc0 = emit_cond(0, -1);
        if (Sink::failed(rc0)) return rc0;
    }
    for (int st = 0; st < h->S; ++st) {
        const int cur = st & 1, nxt = cur ^ 1, par = st & 1;
        const bool produce = st >= nc - 1;
        const StepIo io = step_io(h, view, bv, st);
        const int *u_cc = u_cc_all[par], *u_cl = u_cl_all[par];
        const int last_at_entry = last;     // terminal unit of step st - 1: the guard of step st + 1's tables

        // ---- encoder / decoder
        const float *x = nullptr; long long x_bs = 0; int u_x = last;      // output of the previous layer, its producer
        int u_out[8];
        const float *out_ptr[8]; long long out_bs[8];
        for (int i = 0; i < s->nl; ++i) {
            const S3Layer &l = s->L[i];
            const long long px = (long long)l.ho * l.wo;
            float *ebuf = l.e + row * px * l.C;
            int u_conv;
            if (!l.dec) {
                ConvParams p;
                if (i == 0) {
                    SegArg s1 = plain(vd.ctx_frames, 0);        // the FIRST context frame, shared by every sample
                    p = params(l.conv, plain(io.frame, io.frame_bs), &s1);
                } else {
                    p = params(l.conv, plain(x, x_bs), nullptr);
                }
                p.out = ebuf;
                VF_EMIT(uc, sink.conv(l.conv.G == 4 ? PH_CONV_RAW3G4 : (l.conv.G == 2 ? PH_CONV_RAW3G2 : PH_CONV_RAW3), l.conv, p, {u_x}))
                u_conv = uc;
            } else {
                float *ubuf = l.u + row * px * l.cin;
                EwParams q = ew_base(EW_UPSAMPLE, l.up_items, 0);
                q.up.in0 = x; q.up.in0_bs = x_bs; q.up.C0 = l.c_prev;
                q.up.in1 = l.skip >= 0 ? out_ptr[l.skip] : nullptr; q.up.in1_bs = l.skip >= 0 ? out_bs[l.skip] : 0; q.up.C1 = l.c_skip;
                q.up.out = ubuf; q.up.out_bs = px * l.cin; q.up.h = l.hi; q.up.w = l.wi; q.up.rows = l.up_rows;
                VF_EMIT(uu, sink.ew(q, view, {u_x, l.skip >= 0 ? u_out[l.skip] : -1}))
                ConvParams p = params(l.conv, plain(ubuf, px * l.cin), nullptr);
                p.out = ebuf;
                VF_EMIT(uc, sink.conv(l.conv.G == 4 ? PH_CONV_RAW3G4 : (l.conv.G == 2 ? PH_CONV_RAW3G2 : PH_CONV_RAW3), l.conv, p, {uu}))
                u_conv = uc;
            }
            EwParams q = ew_base(EW_INORM, l.C / l.cpi_n, 0);
            q.norm.in = ebuf; q.norm.in_bs = px * l.C; q.norm.out = ebuf; q.norm.out_bs = px * l.C;
            q.norm.cond = l.cb_conv + ((size_t)par * BV + row) * 25 * l.C; q.norm.cond_bs = 25LL * l.C;
            q.norm.g0 = vw.ng[i]; q.norm.b0 = vw.nb[i];
            q.norm.H = l.ho; q.norm.W = l.wo; q.norm.C = l.C; q.norm.cpi = l.cpi_n; q.norm.relu = 1; q.norm.eps = kS3Eps;
            VF_EMIT(un, sink.ew(q, view, {u_conv, u_cc[i]}))
            x = ebuf; x_bs = px * l.C; u_x = un;
            // The class-bias tables of step st + 1 (fourteen phases of four-sample items; their producers - this step's state
            // FC, the frames of step st - 1 - are long done): behind the smallest encoder layer's conv in ticket order, where a
            // step's phases are narrowest and slots idle.  (Behind the FIRST conv they stood between every sample's first layer
            // and its first gate GEMM: 64 x 64 x 200 samples 75.0 -> 73.2 ms with the move, the C5 shard unchanged.)
            if (i == s->n_enc - 1 && st + 1 < h->S) {
                const int rcn = emit_cond(st + 1, last_at_entry);
                if (Sink::failed(rcn)) return rcn;
            }
            if (l.rnn) {
                float *gates = l.gates + row * px * 4 * l.C;
                float *cbuf = l.c + row * px * l.C;
                float *h_in = l.hst[cur] + row * px * l.C, *h_out = l.hst[nxt] + row * px * l.C;
                SegArg hs = plain(h_in, px * l.C), xs = plain(ebuf, px * l.C);
                ConvParams p = params(l.lstm, hs, &xs);         // recurrent input first (early start)
                p.out = gates;
                if (st == 0) p.chunk_begin = l.lstm.nchunk[0];      // h(-1) = 0: the recurrent chunks multiply zeros
                VF_EMIT(ug, sink.conv_late(PH_GATES_RAW, l.lstm, p, u_cell_prev[i], un))
                EwParams r = ew_base(EW_INCELL, l.C / l.cpi_c, 0);
                r.norm.in = gates; r.norm.in_bs = px * 4 * l.C;
                r.norm.cond = l.cb_lstm + ((size_t)par * BV + row) * 25 * 4 * l.C; r.norm.cond_bs = 25LL * 4 * l.C;
                r.norm.g0 = vw.lg[i]; r.norm.b0 = vw.lb[i]; r.norm.g1 = vw.cg[i]; r.norm.b1 = vw.cb[i];
                r.norm.cprev = st == 0 ? nullptr : cbuf; r.norm.cprev_bs = px * l.C;
                r.norm.out = h_out; r.norm.out_bs = px * l.C; r.norm.cout = cbuf; r.norm.cout_bs = px * l.C;
                r.norm.H = l.ho; r.norm.W = l.wo; r.norm.C = l.C; r.norm.cpi = l.cpi_c; r.norm.eps = kS3Eps;
                VF_EMIT(ucell, sink.ew(r, view, {ug, u_cl[i]}))
                u_cell_prev[i] = ucell;
                x = h_out; x_bs = px * l.C; u_x = ucell;
            }
            u_out[i] = u_x; out_ptr[i] = x; out_bs[i] = x_bs;
        }
        last2 = last;
        last = u_x;
        if (!produce) continue;

        // ---- CDNA kernels from the smallest encoder layer
        const int ib = s->n_enc - 1;
        const ConvLayer &fc_l = Sink::fc_plan(h);
        ConvParams pf = params(fc_l, plain(out_ptr[ib], out_bs[ib]), nullptr);
        pf.out = bv.fc_part;
        VF_EMIT(u_fc, sink.conv(PH_FC_PARTIAL, fc_l, pf, {u_out[ib]}))
        FinParams fp;
        fp.partial = pf.out; fp.nsplit = h->fc.nsplit; fp.B = B; fp.K = h->K;
        fp.bias = vd.b_fc; fp.kern = bv.kern;
        VF_EMIT(u_fin, sink.fin(fp, {u_fc}))

        // ---- heads
        const float *top = x; const long long top_bs = x_bs; const int u_top = u_x;
        float *hm_o = s->hm_o + row * HW * kS3Ngf, *hs_o = s->hs_o + row * HW * kS3Ngf;
        float *scr = s->scr_raw + row * HW * kScrCh, *trans = s->trans + row * HW * kTransCh;
        float *transd = s->transd + row * HW * kNumWarp3 * ND, *mlog = s->mlog + row * HW * kMaskCh;
        float *hmhs_raw = s->hmhs_raw + row * HW * 2 * kS3Ngf;
        ConvParams ph = params(s->hmhs, plain(top, top_bs), nullptr);
        ph.out = hmhs_raw;
        VF_EMIT(u_hc, sink.conv(PH_CONV_RAW3G2, s->hmhs, ph, {u_top}))
        EwParams tq = ew_base(EW_TRANSFORM, h->ntiles, 0);
        tq.top.H = H; tq.top.W = W; tq.top.ND = ND;
        tq.top.prev_frame = io.frame; tq.top.prev_frame_bs = io.frame_bs;
        tq.top.prev_distrib = io.prev_distrib; tq.top.prev_distrib_bs = io.prev_distrib_bs; tq.top.prev_sums = io.prev_sums;
        tq.top.first_frame = vd.ctx_frames; tq.top.first_distrib = vd.ctx_distrib;
        tq.top.kern = fp.kern; tq.top.scr_raw = scr; tq.top.trans = trans; tq.top.transd = transd; tq.top.mlog = mlog;
        tq.top.out_frame = io.out_frame; tq.top.out_frame_bs = io.out_frame_bs;
        tq.top.out_distrib = io.out_distrib; tq.top.out_distrib_bs = io.out_distrib_bs; tq.top.out_sums = io.out_sums;
        set_goal(tq.top.goal, goal_pix, ND);
        const int cpi_h = s3_cpi(H * W, kS3Ngf);
        EwParams nq = ew_base(EW_INORM, 2 * kS3Ngf / cpi_h, 0);
        nq.norm.in = hmhs_raw; nq.norm.in_bs = HW * 2 * kS3Ngf;
        nq.norm.g0 = vw.hmhs_g; nq.norm.b0 = vw.hmhs_b;
        nq.norm.H = H; nq.norm.W = W; nq.norm.C = 2 * kS3Ngf; nq.norm.cpi = cpi_h; nq.norm.relu = 1; nq.norm.eps = kS3Eps;
        if (h->fuse_top) {
            // The heads' second phase as ONE item per 8 x 16-pixel tile (EW_TOP3, vf_savp3.h): the instance norm of the hidden
            // layers only takes its statistics (table of 64 (scale, shift) pairs per sample), the item normalises while staging
            nq.norm.out = hmhs_raw; nq.norm.out_bs = HW * 2 * kS3Ngf;      // (not written: statistics only)
            nq.norm.tab = s->norm_tab + row * 128;
            VF_EMIT(u_tab, sink.ew(nq, view, {u_hc}))
            EwParams f3 = tq;
            f3.op = EW_TOP3;
            f3.gx = ((H + kT3H - 1) / kT3H) * ((W + kT3W - 1) / kT3W);
            f3.top.hmhs_raw = hmhs_raw; f3.top.norm_tab = nq.norm.tab;
            f3.top.w_scr = vw.w_scr_v; f3.top.b_scr = vw.b_scr_v; f3.top.w_msk = vw.w_msk_v; f3.top.b_msk = vw.b_msk_v;
            VF_EMIT(u_f3, sink.ew(f3, view, {u_tab, u_fin, last2}))
            last = u_f3;
            continue;
        }
        // (vf_set_fuse_top(0): the four-phase form - scratch conv, layers, mask conv, composition - through memory)
        nq.norm.out = hm_o; nq.norm.out2 = hs_o; nq.norm.split = kS3Ngf; nq.norm.out_bs = HW * kS3Ngf;
        VF_EMIT(u_hn, sink.ew(nq, view, {u_hc}))
        ConvParams ps = params(s->scratch, plain(hs_o, HW * kS3Ngf), nullptr);
        ps.out = scr;
        VF_EMIT(u_scr, sink.conv(PH_CONV_RAW3, s->scratch, ps, {u_hn}))
        VF_EMIT(u_tr, sink.ew(tq, view, {u_scr, u_fin, last2}))
        SegArg ts = plain(trans, HW * kTransCh);
        ConvParams pm = params(s->masks, plain(hm_o, HW * kS3Ngf), &ts);
        pm.out = mlog;
        VF_EMIT(u_m, sink.conv(PH_CONV_RAW3, s->masks, pm, {u_hn, u_tr}))
        EwParams cq = tq;
        cq.op = EW_COMPOSE;
        VF_EMIT(u_comp, sink.ew(cq, view, {u_m, u_tr}))
        last = u_comp;
    }
    return VF_OK;
}

}  // namespace vf
