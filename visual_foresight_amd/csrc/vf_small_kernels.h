// vf_small_kernels.h - the non-GEMM kernels of one predictor step (all fp32 VALU, HBM/LDS bound):
//   set_context      uint8 context frames -> float/255, context copies
//   sa_kernel        state FC + the action/state part of enc3 as a per-sample bias
//   cdna_finalize    sum K-split partials of the CDNA FC, relu-shift, L1-normalise each 5x5 kernel
//   stp_finalize     sum K-split partials of the STP head's first FC, relu, second FC, the nine transforms in pixel units
//   composite        LN9+relu -> rgb/mask heads -> softmax -> CDNA warp -> compositing of the next
//                    frame and designated-pixel distributions + expected-distance partial sums
//   scores / export  reduce per-step sums to costs (mean over tasks or trade-off weights, mean over
//                    latent draws); hand predictions out in the reference layout (camera axis)
//   ensemble_scores  the same reduction over E engines' sums, per step mean + lambda * variance over the members
//   register         bilinear warp by a flow field + designated-pixel re-localisation + warp error
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vf_conv_mfma.h"

namespace vf {

constexpr int kMaxDesig = 4;
// Extent of an array with one entry per designated pixel.  A frames-only item (ND = 0) has no such values:
// every loop over them runs zero times and every access sits behind `if constexpr (ND > 0)`, so the one slot that keeps the
// array type well-formed is never read or written and costs no register.  For ND >= 1 the extent is ND itself.
__host__ __device__ constexpr int nd_slots(int nd) { return nd > 0 ? nd : 1; }
constexpr int kDnaKern = 5;
constexpr int kTaps = kDnaKern * kDnaKern;
constexpr int kCompTile = 16;           // composite: 16x16 pixels per workgroup
// Cost sums are kept per BLOCK of 4 rows x 16 columns - the pixels one wave of a compositing tile handles - and
// added up in block order by their readers, so the decomposition of an image into workgroup tiles does not show
// in the sums (any tiling whose waves cover whole blocks gives the same bits).
constexpr int kSumBlockH = 4, kSumBlockW = 16;
__host__ __device__ constexpr int sum_blocks_x(int W) { return (W + kSumBlockW - 1) / kSumBlockW; }
__host__ __device__ constexpr int sum_blocks(int H, int W) { return ((H + kSumBlockH - 1) / kSumBlockH) * sum_blocks_x(W); }
constexpr float kReluShift = 1e-12f;

// ------------------------------------------------------------------------------------------
// frames_u8 [nc][ncam][HW3] -> frames_f [ncam][nc][HW3] / 255; distrib [nc][ncam][HWD] -> [ncam][nc][HWD];
// states and context actions are shared by the views and copied as they are
VF_GLOBAL void set_context_kernel(const uint8_t *frames_u8, float *frames_f, int nc, int ncam, int hw3,
                                   const float *src_d, float *dst_d, int hwd,
                                   const float *src_s, float *dst_s, int n_s,
                                   const float *src_a, float *dst_a, int n_a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nc * ncam * hw3) {
        const int e = i % hw3, v = (i / hw3) % ncam, t = i / (hw3 * ncam);
        frames_f[((long long)v * nc + t) * hw3 + e] = (float)frames_u8[i] / 255.0f;
    }
    if (i < nc * ncam * hwd) {
        const int e = i % hwd, v = (i / hwd) % ncam, t = i / (hwd * ncam);
        dst_d[((long long)v * nc + t) * hwd + e] = src_d[i];
    }
    if (i < n_s) dst_s[i] = src_s[i];
    if (i < n_a) dst_a[i] = src_a[i];
}

// Grouped contexts (vf_set_contexts): G contexts in the caller's layout, [G][nc][ncam][..], converted as above and EXPANDED
// into one copy per row - row g * rpg + j of every buffer holds context g:
//   frames_f [ncam][G * rpg][nc][HW3], dst_d [ncam][G * rpg][nc][HWD], dst_s [G * rpg][n_s], dst_a [G * rpg][n_a]
// (n_s = nc * sdim, n_a = (nc - 1) * adim), so that a step reads its context as `ptr + row * stride` exactly where it reads
// a rolled input.  One thread per OUTPUT element of the largest buffer; every value is the one set_context_kernel writes.
VF_GLOBAL void set_contexts_kernel(const uint8_t *frames_u8, float *frames_f, int G, int rpg, int nc, int ncam, int hw3,
                                    const float *src_d, float *dst_d, int hwd,
                                    const float *src_s, float *dst_s, int n_s,
                                    const float *src_a, float *dst_a, int n_a) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long rows = (long long)G * rpg;
    if (i < (long long)ncam * rows * nc * hw3) {
        const int e = (int)(i % hw3), t = (int)((i / hw3) % nc);
        const long long row = (i / ((long long)hw3 * nc)) % rows, v = i / ((long long)hw3 * nc * rows);
        frames_f[i] = (float)frames_u8[(((row / rpg) * nc + t) * ncam + v) * hw3 + e] / 255.0f;
    }
    if (i < (long long)ncam * rows * nc * hwd) {
        const int e = (int)(i % hwd), t = (int)((i / hwd) % nc);
        const long long row = (i / ((long long)hwd * nc)) % rows, v = i / ((long long)hwd * nc * rows);
        dst_d[i] = src_d[(((row / rpg) * nc + t) * ncam + v) * hwd + e];
    }
    if (i < rows * n_s) dst_s[i] = src_s[((i / n_s) / rpg) * n_s + i % n_s];
    if (i < rows * n_a) dst_a[i] = src_a[((i / n_a) / rpg) * n_a + i % n_a];
}

// ------------------------------------------------------------------------------------------
struct SaParams {
    const float *action; long long action_bstride;     // [adim] per sample (0 stride: shared)
    const float *state;  long long state_bstride;      // [sdim]
    int adim, sdim, B;
    const float *w_state, *b_state;     // [adim+sdim][sdim], [sdim]
    const float *w_sa;                  // enc3 rows for the smeared inputs: [adim+sdim][n_out]
    int n_out;                          // 64
    float *state_out; long long state_out_bstride;      // may be null
    float *sbias;                       // [B][n_out]
};

// one sample, executed by the 64 lanes of one wave; sa = 32 floats of LDS scratch for this wave
template <class PT>
__device__ __forceinline__ void sa_sample(const PT &p, const int b, const int t, float *sa) {
    const int nsa = p.adim + p.sdim;
    if (t < p.adim) sa[t] = p.action[(long long)b * p.action_bstride + t];
    else if (t < nsa) sa[t] = p.state[(long long)b * p.state_bstride + (t - p.adim)];
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    if (t < p.n_out) {
        float acc = 0.f;
        for (int k = 0; k < nsa; ++k) acc = fmaf(sa[k], p.w_sa[k * p.n_out + t], acc);
        p.sbias[(long long)b * p.n_out + t] = acc;
    }
    if (p.state_out && t < p.sdim) {
        float acc = 0.f;
        for (int k = 0; k < nsa; ++k) acc = fmaf(sa[k], p.w_state[k * p.sdim + t], acc);
        p.state_out[(long long)b * p.state_out_bstride + t] = acc + p.b_state[t];
    }
}

VF_GLOBAL void sa_kernel(const SaParams p) {
    __shared__ float sa[32];
    sa_sample(p, blockIdx.x, threadIdx.x, sa);
}

// ------------------------------------------------------------------------------------------
// kern[b][tap][k] = v / sum_tap v,  v = relu(fc - shift) + shift,  fc = bias + sum_split partial
struct FinParams {
    const float *partial; int nsplit; int B; int K;
    const float *bias; float *kern;
};

// one sample per workgroup call; scratch: kTaps*16 + 16 floats of LDS
template <class PT>
__device__ __forceinline__ void cdna_finalize_sample(const PT &p, const int b, float *scratch) {
    const int t = threadIdx.x;
    const int n = kTaps * p.K;
    float *v = scratch, *norm = scratch + kTaps * 16;
    if (t < n) {
        float acc = p.bias[t];
        for (int z = 0; z < p.nsplit; ++z) acc += p.partial[((long long)z * p.B + b) * n + t];
        v[t] = fmaxf(acc - kReluShift, 0.f) + kReluShift;
    }
    __syncthreads();
    if (t < p.K) {
        float s = 0.f;
        for (int tap = 0; tap < kTaps; ++tap) s += v[tap * p.K + t];
        norm[t] = s;
    }
    __syncthreads();
    if (t < n) p.kern[(long long)b * n + t] = v[t] / norm[t % p.K];
}

VF_GLOBAL void cdna_finalize_kernel(const FinParams p) {
    __shared__ float scratch[kTaps * 16 + 16];
    cdna_finalize_sample(p, blockIdx.x, scratch);
}

// ------------------------------------------------------------------------------------------
// Per-layer conditioning of arch 2 (savp_arch.py, Savp2Config): the published SAVP generator tiles the vector
// v = [action, latent, state] over the image and concatenates it to the input of EVERY conv-LSTM (arXiv:1804.01523,
// appendix A).  A spatially constant input channel needs no GEMM rows: with zero padding its contribution to gate column
// `col` at pixel (y, x) is  sum over the taps (dy, dx) that fall inside the image of  t[dy][dx][col],
// t[tap][col] = sum_c W[tap][c][col] v[c],  and which taps fall inside only depends on whether y (x) is one of the two
// first / two last rows (columns): 5 x 5 border classes.  One item per (conv-LSTM, sample) computes the 25 class biases for
// all 4C gate columns; the conv-LSTM epilogue adds the row of its pixel's class.  No K growth (as real channels the 17
// values would cost every cell one more 32-channel chunk: +17 ... +50 % matrix work), same sums as the concatenated
// convolution up to fp32 association.
struct CondParams {
    const float *action; long long action_bstride;     // [adim] per sample (latent channels included; 0 stride: shared)
    const float *state;  long long state_bstride;      // [sdim]
    int adim, sdim, B;
    const float *w;         // [25 taps][adim + sdim][C4]: the conditioning rows of the layer's canonical weights
    int C4;                 // 4 * cell channels (gate-major columns)
    float *out;             // [B][25 classes][C4]
};
constexpr int kCondClasses = kTaps;
// border class of coordinate y in an image of H rows (5-tap kernel, pad 2): 0, 1 | 2 = interior | 3, 4
__host__ __device__ constexpr int cond_class(int y, int H) { return y < 2 ? y : (y >= H - 2 ? y - (H - 5) : 2); }
// first / one-past-last kernel tap that reads inside the image for class r
__host__ __device__ constexpr int cond_tap_lo(int r) { return r < 2 ? 2 - r : 0; }
__host__ __device__ constexpr int cond_tap_hi(int r) { return r > 2 ? 7 - r : 5; }

// samples [b0, b1) (at most kCondPerItem) per workgroup call; sv = kCondPerItem * 32 floats of LDS scratch.  A weight is
// loaded once for all samples of the call; every sample's sums run in the same order as in a one-sample call (same bits).
constexpr int kCondPerItem = 4;
template <class PT>
__device__ __forceinline__ void cond_bias_sample(const PT &p, const int b0, const int b1, float *sv) {
    const int t = threadIdx.x, nsa = p.adim + p.sdim, ns = b1 - b0;
    if (t < kCondPerItem * 32) {
        const int s = t >> 5, c = t & 31;
        float v = 0.f;
        if (s < ns) {
            if (c < p.adim) v = p.action[(long long)(b0 + s) * p.action_bstride + c];
            else if (c < nsa) v = p.state[(long long)(b0 + s) * p.state_bstride + (c - p.adim)];
        }
        sv[t] = v;
    }
    __syncthreads();
    for (int col = t; col < p.C4; col += 256) {
        float tt[kCondPerItem][kTaps];
#pragma unroll
        for (int tap = 0; tap < kTaps; ++tap) {
            float acc[kCondPerItem];
#pragma unroll
            for (int s = 0; s < kCondPerItem; ++s) acc[s] = 0.f;
            for (int c = 0; c < nsa; ++c) {
                const float w = p.w[((long long)tap * nsa + c) * p.C4 + col];
#pragma unroll
                for (int s = 0; s < kCondPerItem; ++s) acc[s] = fmaf(sv[s * 32 + c], w, acc[s]);
            }
#pragma unroll
            for (int s = 0; s < kCondPerItem; ++s) tt[s][tap] = acc[s];
        }
#pragma unroll
        for (int s = 0; s < kCondPerItem; ++s) {
            if (s >= ns) break;
            // row sums over the columns of class rx, then over the rows of class ry (fixed order: deterministic)
            float S[5][5];
#pragma unroll
            for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                for (int rx = 0; rx < 5; ++rx) {
                    float a = 0.f;
#pragma unroll
                    for (int dx = 0; dx < 5; ++dx)
                        if (dx >= cond_tap_lo(rx) && dx < cond_tap_hi(rx)) a += tt[s][dy * 5 + dx];
                    S[dy][rx] = a;
                }
            float *o = p.out + (long long)(b0 + s) * kCondClasses * p.C4 + col;
#pragma unroll
            for (int ry = 0; ry < 5; ++ry)
#pragma unroll
                for (int rx = 0; rx < 5; ++rx) {
                    float a = 0.f;
#pragma unroll
                    for (int dy = 0; dy < 5; ++dy)
                        if (dy >= cond_tap_lo(ry) && dy < cond_tap_hi(ry)) a += S[dy][rx];
                    o[(long long)(ry * 5 + rx) * p.C4] = a;
                }
        }
    }
}

VF_GLOBAL VF_LAUNCH_BOUNDS(256) void cond_bias_kernel(const CondParams p) {
    __shared__ float sv[kCondPerItem * 32];
    const int b0 = blockIdx.x * kCondPerItem;
    cond_bias_sample(p, b0, min(b0 + kCondPerItem, p.B), sv);
}

// ------------------------------------------------------------------------------------------
struct CompositeParams {
    int B, H, W, ND, K;                 // K = num_masks (K+1 mask channels, K-1 kernels used)
    const float *enc6;                  // raw convT3 output [B][H][W][32]
    const long long *ln_part; int ln_nparts; float ln_inv_n;     // exact statistics of enc6 (vf_conv_mfma.h)
    const float *gamma, *beta;          // LN9 [32]
    const float *w_rgb, *b_rgb;         // [32][3], [3]
    const float *w_mask, *b_mask;       // [32][K+1], [K+1]
    const float *kern;                  // [B][25][K]; STP engines (stp_arch.py): the sample's transforms [B][kStpWarps][6]
    const float *prev_frame; long long prev_frame_bstride;      // [H][W][3]
    const float *prev_distrib; long long prev_distrib_bstride;  // [H][W][ND]
    const double *prev_sums;            // [B][ND][blocks][2] partial sums of prev_distrib, or null
    const float *first_frame;           // arch 1 (savp_arch.py): first context frame [H][W][3], shared by every
    const float *first_distrib;         //   sample, and its distributions [H][W][ND]; null = CDNA compositing
    float *out_frame; long long out_frame_bstride;
    float *out_distrib; long long out_distrib_bstride;
    double *out_sums;                   // [B][ND][blocks][2]: sum d, sum d * dist(goal) per 4x16-pixel block
    int goal[kMaxDesig][2];             // (row, col); read by the per-layer kernel only - the persistent
                                        // kernel takes the goals from its launch arguments, so a schedule
                                        // does not depend on them
    int CF;                             // feature channels of enc6: 0 / 32, or 64 (the public CDNA decoder table, cdna_arch.py
                                        // decoder='public': the stand-alone compositing tile only, two 32-channel rounds)
    const float *w_head, *b_head;       // the mode's own 1x1 head (`kern` is null there): appearance-flow engines (cdna_arch.py
                                        // transformation='flow') the flow head [32][2 * kFlowWarps], [2 * kFlowWarps]; DNA engines
                                        // (dna_arch.py, K == 1) the kernel head [32][kTaps], [kTaps].  Null = CDNA kernels / STP.
};

// LDS floats needed by composite_tile<ND, K>
constexpr int kCompEncPad = 36;         // floats per pixel row of the staged feature tile (32 + 4: conflict-free b128 reads)
// The haloed previous frame and distributions sit in LDS as ONE record per pixel - [r, g, b, d0 | d1, d2, d3, -] - and
// the sample's CDNA kernels as one 12-float row per tap, so the 25 taps of a pixel cost 25 x (1 or 2) + 25 x 3
// ds_read_b128 / b32 instead of 25 x (3 + ND) + 25 x 9 ds_read_b32: the compositing is LDS-instruction bound.
__host__ __device__ constexpr int comp_px_stride(int nd) { return nd <= 1 ? 4 : 8; }
constexpr int kCompKernPad = 12;        // floats per tap row of the CDNA kernels in LDS (K <= 10 used, 16-byte aligned rows)
template <int ND, int K>
__host__ __device__ constexpr int composite_small_floats() {
    return (kCompTile + 4) * (kCompTile + 4) * comp_px_stride(ND) + kTaps * kCompKernPad + 2 + ND + 2 /*pad*/ + 2 * 4 * 2 * ND;
}
template <int ND, int K>
__host__ __device__ constexpr int composite_lds_floats() {
    return ((composite_small_floats<ND, K>() + 3) & ~3) + kCompTile * kCompTile * kCompEncPad;
}

// The two 1x1 heads of one pixel, accumulated over 32 feature channels [c_off, c_off + 32) of the LDS feature row `feat`
// (LN + relu applied on the way).  The 512 head / LayerNorm weights are the same for every lane: read through the CONSTANT
// address space they are scalar loads feeding the VALU as SGPR operands - as plain global pointers the compiler issued 132
// vector loads (and as many waits) per pixel, which was half of the compositing time.
template <int K, class PT>
__device__ __forceinline__ void composite_head_bias(const PT &p, float (&o_rgb)[3], float (&o_m)[K + 1]) {
    typedef const __attribute__((address_space(4))) float cfloat;
    cfloat *brgb_ = (cfloat *)(unsigned long long)p.b_rgb, *bmask_ = (cfloat *)(unsigned long long)p.b_mask;
#pragma unroll
    for (int j = 0; j < 3; ++j) o_rgb[j] = brgb_[j];
#pragma unroll
    for (int j = 0; j < K + 1; ++j) o_m[j] = bmask_[j];
}
template <int K, class PT>
__device__ __forceinline__ void composite_heads(const PT &p, const float *feat, const float mean, const float rstd,
                                                const int c_off, float (&o_rgb)[3], float (&o_m)[K + 1]) {
    constexpr int NM = K + 1;
    typedef const __attribute__((address_space(4))) float cfloat;
    auto as_const = [](const float *q) { return (cfloat *)(unsigned long long)q; };
    cfloat *gam_ = as_const(p.gamma) + c_off, *bet_ = as_const(p.beta) + c_off;
    cfloat *wrgb_ = as_const(p.w_rgb) + c_off * 3, *wmask_ = as_const(p.w_mask) + c_off * NM;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(feat);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 raw = src[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = q * 4 + e;
            const float f = fmaxf(fmaf((raw[e] - mean) * rstd, gam_[c], bet_[c]), 0.f);
#pragma unroll
            for (int j = 0; j < 3; ++j) o_rgb[j] = fmaf(f, wrgb_[c * 3 + j], o_rgb[j]);
#pragma unroll
            for (int j = 0; j < NM; ++j) o_m[j] = fmaf(f, wmask_[c * NM + j], o_m[j]);
        }
    }
}
template <int ND, int K, bool FIRST, class PT>
__device__ __forceinline__ void composite_finish(const PT &p, const int b, const int y, const int x, float (&o_rgb)[3],
                                                 float (&o_m)[K + 1], const float *s_px, const float *s_kern, const int halo_w,
                                                 const int hy, const int hx, const int *goal, double (&cost)[2 * nd_slots(ND)]);
template <int ND, int K, bool FIRST, class PT>
__device__ __forceinline__ void composite_values(const PT &p, const int y, const int x, float (&o_rgb)[3],
                                                 float (&o_m)[K + 1], const float *s_px, const float *s_kern, const int halo_w,
                                                 const int hy, const int hx, const int *goal, double (&cost)[2 * nd_slots(ND)],
                                                 float (&of)[3], float (&od)[nd_slots(ND)]);

// One output pixel (y, x) of sample b: LN + relu of its 32 features (a row of the LDS feature tile), the two 1x1
// heads, softmax, the effective 5x5 flow kernel over the haloed previous frame / distributions in LDS
// (halo_w = pixels per halo row, (hy, hx) = the pixel's position inside the halo tile, halo 2), outputs and cost terms.
// Shared by the stand-alone compositing tile and the fused transposed-conv + compositing tile: same expressions,
// same bits.
template <int ND, int K, bool FIRST, class PT>
__device__ __forceinline__ void composite_pixel(const PT &p, const int b, const int y, const int x, const float *feat,
                                                const float mean, const float rstd, const float *s_px,
                                                const float *s_kern, const int halo_w,
                                                const int hy, const int hx, const int *goal, double (&cost)[2 * nd_slots(ND)]) {
    constexpr int NM = K + 1;
    static_assert(K <= 10 && ND <= 4, "LDS record layouts");
    float o_rgb[3], o_m[NM];
    composite_head_bias<K>(p, o_rgb, o_m);
    composite_heads<K>(p, feat, mean, rstd, 0, o_rgb, o_m);
    composite_finish<ND, K, FIRST>(p, b, y, x, o_rgb, o_m, s_px, s_kern, halo_w, hy, hx, goal, cost);
}
// ... its next-frame pixel and distributions returned instead of stored (the fused top turns a block over in LDS and
// stores whole 16-byte pieces write-through: vf_fused_top.h) - the same expressions, the same bits
template <int ND, int K, bool FIRST, class PT>
__device__ __forceinline__ void composite_pixel_values(const PT &p, const int y, const int x, const float *feat,
                                                       const float mean, const float rstd, const float *s_px,
                                                       const float *s_kern, const int halo_w, const int hy, const int hx,
                                                       const int *goal, double (&cost)[2 * nd_slots(ND)], float (&of)[3], float (&od)[nd_slots(ND)]) {
    constexpr int NM = K + 1;
    float o_rgb[3], o_m[NM];
    composite_head_bias<K>(p, o_rgb, o_m);
    composite_heads<K>(p, feat, mean, rstd, 0, o_rgb, o_m);
    composite_values<ND, K, FIRST>(p, y, x, o_rgb, o_m, s_px, s_kern, halo_w, hy, hx, goal, cost, of, od);
}

// the part of a pixel behind its head outputs: softmax, effective flow kernel, next frame / distributions, cost terms
template <int ND, int K, bool FIRST, class PT>
__device__ __forceinline__ void composite_finish(const PT &p, const int b, const int y, const int x, float (&o_rgb)[3],
                                                 float (&o_m)[K + 1], const float *s_px, const float *s_kern, const int halo_w,
                                                 const int hy, const int hx, const int *goal, double (&cost)[2 * nd_slots(ND)]) {
    float of[3], od[nd_slots(ND)];
    composite_values<ND, K, FIRST>(p, y, x, o_rgb, o_m, s_px, s_kern, halo_w, hy, hx, goal, cost, of, od);
    const long long o = (long long)y * p.W + x;
    float *fo = p.out_frame + (long long)b * p.out_frame_bstride + o * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) fo[c] = of[c];
    if constexpr (ND > 0) {
        float *dout = p.out_distrib + (long long)b * p.out_distrib_bstride + o * ND;
#pragma unroll
        for (int d = 0; d < ND; ++d) dout[d] = od[d];
    }
}
template <int ND, int K, bool FIRST, class PT>
__device__ __forceinline__ void composite_values(const PT &p, const int y, const int x, float (&o_rgb)[3],
                                                 float (&o_m)[K + 1], const float *s_px, const float *s_kern, const int halo_w,
                                                 const int hy, const int hx, const int *goal, double (&cost)[2 * nd_slots(ND)],
                                                 float (&of)[3], float (&od)[nd_slots(ND)]) {
    constexpr int NM = K + 1;
    constexpr int PS = comp_px_stride(ND);
    auto load_px = [&](const int sp, float (&fr)[3], float (&di)[nd_slots(ND)]) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(s_px + sp * PS);
        fr[0] = a[0]; fr[1] = a[1]; fr[2] = a[2];
        if constexpr (ND > 0) di[0] = a[3];
        if constexpr (ND > 1) {
            const f32x4 c2 = *reinterpret_cast<const f32x4 *>(s_px + sp * PS + 4);
#pragma unroll
            for (int d = 1; d < ND; ++d) di[d] = c2[d - 1];
        }
    };
    float mx = o_m[0];
#pragma unroll
    for (int j = 1; j < NM; ++j) mx = fmaxf(mx, o_m[j]);
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < NM; ++j) { o_m[j] = __expf(o_m[j] - mx); den += o_m[j]; }
    const float inv = 1.0f / den;
#pragma unroll
    for (int j = 0; j < NM; ++j) o_m[j] *= inv;

    // ---- per-pixel effective flow kernel: keff[tap] = sum_k mask[k+2] * kern[tap][k]
    // (arch 1: mask 2 weighs the first context frame, the warps use masks 3.. and kernels 0..K-3)
    const int ctr = (hy + 2) * halo_w + (hx + 2);
    {
        float fr[3], di[nd_slots(ND)];
        load_px(ctr, fr, di);
#pragma unroll
        for (int c = 0; c < 3; ++c) of[c] = fmaf(o_m[0], fr[c], o_m[1] * sigmoidf_(o_rgb[c]));
        // (K == 6, arch 2: the published generator composes the distributions with the PREVIOUS distribution in the
        // scratch layer's slot too - the scratch image has no distribution of its own)
#pragma unroll
        for (int d = 0; d < ND; ++d) od[d] = (K == 6 ? o_m[0] + o_m[1] : o_m[0]) * di[d];
    }
    if constexpr (FIRST) {
        const long long o1 = (long long)y * p.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) of[c] = fmaf(o_m[2], p.first_frame[o1 * 3 + c], of[c]);
#pragma unroll
        for (int d = 0; d < ND; ++d) od[d] = fmaf(o_m[2], p.first_distrib[o1 * ND + d], od[d]);
        // the warp loop below pairs kernel k with o_m[k + 2]: shift the warp masks down by one and
        // retire the last kernel (its product with 0 leaves the sum unchanged)
#pragma unroll
        for (int j = 2; j < K; ++j) o_m[j] = o_m[j + 1];
        o_m[K] = 0.f;
    }
#pragma unroll
    for (int dy = 0; dy < kDnaKern; ++dy) {
#pragma unroll
        for (int dx = 0; dx < kDnaKern; ++dx) {
            const int tap = dy * kDnaKern + dx;
            float kr[kCompKernPad];
#pragma unroll
            for (int q = 0; q < (K - 1 + 3) / 4; ++q) {
                const f32x4 kq = *reinterpret_cast<const f32x4 *>(s_kern + tap * kCompKernPad + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) kr[4 * q + e] = kq[e];
            }
            float ke = 0.f;
#pragma unroll
            for (int k = 0; k < K - 1; ++k) ke = fmaf(o_m[k + 2], kr[k], ke);
            const int sp = (hy + dy) * halo_w + (hx + dx);
            float fr[3], di[nd_slots(ND)];
            load_px(sp, fr, di);
#pragma unroll
            for (int c = 0; c < 3; ++c) of[c] = fmaf(ke, fr[c], of[c]);
#pragma unroll
            for (int d = 0; d < ND; ++d) od[d] = fmaf(ke, di[d], od[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const float ry = (float)(y - goal[2 * d]), rx = (float)(x - goal[2 * d + 1]);
        const float dist = sqrtf(fmaf(ry, ry, rx * rx));
        cost[2 * d] = (double)od[d];
        cost[2 * d + 1] = (double)od[d] * (double)dist;
    }
}

// ------------------------------------------------------------------------------------------
// Appearance-flow compositing (cdna_arch.py, transformation='flow').  Instead of the sample's CDNA kernels
// a third 1x1 head predicts a displacement (dx_k, dy_k) in pixels per warp k and pixel; warp k samples the previous frame
// and distributions at (x + dx_k, y + dy_k) with the clamped bilinear taps of bilinear_clamped() below.  A tap may lie
// anywhere in the image, so nothing is staged in LDS: the gathers read the sample's previous frame / distributions from
// global memory (L2), which therefore must be COMPLETE before any tile of the step starts - the dependency on the first conv
// of the step, which itself waited for every compositing tile of the previous step, gives that (emit_rollout).
constexpr int kFlowWarps = 9;           // NF = num_masks - 1 warps: the cdna path uses nine of its ten kernels too

// the flow head of one pixel: a SECOND pass over its LDS feature row (with the rgb / mask sums of the first pass that would
// be 32 live accumulators, which the compose pass of the fused top cannot hold for ND > 2).  Every sum is its own fma chain
// over the channels ascending from the bias, as in composite_heads: the split into two passes does not show in the bits.
template <class PT>
__device__ __forceinline__ void composite_flow_heads(const PT &p, const float *feat, const float mean, const float rstd,
                                                     float (&o_fl)[2 * kFlowWarps]) {
    constexpr int NF2 = 2 * kFlowWarps;
    typedef const __attribute__((address_space(4))) float cfloat;
    auto as_const = [](const float *q) { return (cfloat *)(unsigned long long)q; };
    cfloat *gam_ = as_const(p.gamma), *bet_ = as_const(p.beta);
    cfloat *wfl_ = as_const(p.w_head), *bfl_ = as_const(p.b_head);
#pragma unroll
    for (int j = 0; j < NF2; ++j) o_fl[j] = bfl_[j];
    const f32x4 *src = reinterpret_cast<const f32x4 *>(feat);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 raw = src[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = q * 4 + e;
            const float f = fmaxf(fmaf((raw[e] - mean) * rstd, gam_[c], bet_[c]), 0.f);
#pragma unroll
            for (int j = 0; j < NF2; ++j) o_fl[j] = fmaf(f, wfl_[c * NF2 + j], o_fl[j]);
        }
    }
}

// One output pixel (y, x) behind its rgb / mask head outputs: softmax, the flow head, nine gathered warps, next frame /
// distributions, cost terms.  pf / pd: the sample's previous frame [H][W][3] / distributions [H][W][ND] in global memory,
// dscale[d] = 1 / (mass of previous distribution d), applied to every tap before the interpolation (as the halo load of the
// cdna path applies it).  Accumulation order: previous frame, scratch, warps k ascending.  Coordinates are clamped before
// they become indices (a NaN flow clamps to 0), so every gather stays inside the image.
template <int ND, class PT>
__device__ __forceinline__ void composite_values_flow(const PT &p, const int y, const int x, const float *feat,
                                                      const float mean, const float rstd, float (&o_rgb)[3],
                                                      float (&o_m)[kFlowWarps + 2], const float *pf, const float *pd,
                                                      const float *dscale, const int *goal, double (&cost)[2 * nd_slots(ND)],
                                                      float (&of)[3], float (&od)[nd_slots(ND)]) {
    constexpr int NM = kFlowWarps + 2;
    float mx = o_m[0];
#pragma unroll
    for (int j = 1; j < NM; ++j) mx = fmaxf(mx, o_m[j]);
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < NM; ++j) { o_m[j] = __expf(o_m[j] - mx); den += o_m[j]; }
    const float inv = 1.0f / den;
#pragma unroll
    for (int j = 0; j < NM; ++j) o_m[j] *= inv;

    float sc[nd_slots(ND)];
#pragma unroll
    for (int d = 0; d < ND; ++d) sc[d] = dscale[d];
    {
        const long long o = (long long)y * p.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) of[c] = fmaf(o_m[0], pf[o * 3 + c], o_m[1] * sigmoidf_(o_rgb[c]));
#pragma unroll
        for (int d = 0; d < ND; ++d) od[d] = o_m[0] * (pd[o * ND + d] * sc[d]);
    }
    float o_fl[2 * kFlowWarps];
    composite_flow_heads(p, feat, mean, rstd, o_fl);
    const float xmax = (float)(p.W - 1), ymax = (float)(p.H - 1);
#pragma unroll
    for (int k = 0; k < kFlowWarps; ++k) {
        // the taps of bilinear_clamped(), shared by the frame's channels and the distributions
        const float sx = fminf(fmaxf((float)x + o_fl[2 * k], 0.f), xmax);
        const float sy = fminf(fmaxf((float)y + o_fl[2 * k + 1], 0.f), ymax);
        const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
        const int x1 = min(x0 + 1, p.W - 1), y1 = min(y0 + 1, p.H - 1);
        const float fx = sx - (float)x0, fy = sy - (float)y0;
        const int o00 = y0 * p.W + x0, o01 = y0 * p.W + x1, o10 = y1 * p.W + x0, o11 = y1 * p.W + x1;
        const float m = o_m[k + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a = pf[o00 * 3 + c], b = pf[o01 * 3 + c], cc = pf[o10 * 3 + c], dd = pf[o11 * 3 + c];
            const float top = fmaf(fx, b - a, a), bot = fmaf(fx, dd - cc, cc);
            of[c] = fmaf(m, fmaf(fy, bot - top, top), of[c]);
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const float a = pd[o00 * ND + d] * sc[d], b = pd[o01 * ND + d] * sc[d];
            const float cc = pd[o10 * ND + d] * sc[d], dd = pd[o11 * ND + d] * sc[d];
            const float top = fmaf(fx, b - a, a), bot = fmaf(fx, dd - cc, cc);
            od[d] = fmaf(m, fmaf(fy, bot - top, top), od[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const float ry = (float)(y - goal[2 * d]), rx = (float)(x - goal[2 * d + 1]);
        const float dist = sqrtf(fmaf(ry, ry, rx * rx));
        cost[2 * d] = (double)od[d];
        cost[2 * d + 1] = (double)od[d] * (double)dist;
    }
}
// ... from the pixel's LDS feature row (the stand-alone tile and the fused top call this: same expressions, same bits)
template <int ND, class PT>
__device__ __forceinline__ void composite_pixel_values_flow(const PT &p, const int y, const int x, const float *feat,
                                                            const float mean, const float rstd, const float *pf,
                                                            const float *pd, const float *dscale, const int *goal,
                                                            double (&cost)[2 * nd_slots(ND)], float (&of)[3], float (&od)[nd_slots(ND)]) {
    float o_rgb[3], o_m[kFlowWarps + 2];
    composite_head_bias<kFlowWarps + 1>(p, o_rgb, o_m);
    composite_heads<kFlowWarps + 1>(p, feat, mean, rstd, 0, o_rgb, o_m);
    composite_values_flow<ND>(p, y, x, feat, mean, rstd, o_rgb, o_m, pf, pd, dscale, goal, cost, of, od);
}

// ------------------------------------------------------------------------------------------
// DNA compositing (dna_arch.py; arXiv:1605.07157 section 3.1).  A 1x1 head predicts 25 values per PIXEL;
// relu-shifted and normalised they are that pixel's own 5x5 kernel over the previous frame and distributions - where the
// CDNA path mixes the sample's nine kernels by its masks.  One transform, two mask channels (previous frame | transformed),
// no scratch image.  The halo tile in LDS is the CDNA path's; the kernel table is not staged.  The head reaches the device
// through CompositeParams::w_head / b_head ([32][kTaps], [kTaps]) with K == 1.
//
// The two mask sums and the 25 tap sums of one pixel: each its own fma chain over the channels ascending from the bias, on
// f_c = relu(LN9(enc6)_c), as composite_heads builds its sums (27 live accumulators, one pass over the LDS feature row).
template <class PT>
__device__ __forceinline__ void composite_dna_heads(const PT &p, const float *feat, const float mean, const float rstd,
                                                    float (&o_m)[2], float (&o_a)[kTaps]) {
    typedef const __attribute__((address_space(4))) float cfloat;
    auto as_const = [](const float *q) { return (cfloat *)(unsigned long long)q; };
    cfloat *gam_ = as_const(p.gamma), *bet_ = as_const(p.beta);
    cfloat *wmask_ = as_const(p.w_mask), *bmask_ = as_const(p.b_mask);
    cfloat *wdna_ = as_const(p.w_head), *bdna_ = as_const(p.b_head);
#pragma unroll
    for (int j = 0; j < 2; ++j) o_m[j] = bmask_[j];
#pragma unroll
    for (int t = 0; t < kTaps; ++t) o_a[t] = bdna_[t];
    const f32x4 *src = reinterpret_cast<const f32x4 *>(feat);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const f32x4 raw = src[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = q * 4 + e;
            const float f = fmaxf(fmaf((raw[e] - mean) * rstd, gam_[c], bet_[c]), 0.f);
#pragma unroll
            for (int j = 0; j < 2; ++j) o_m[j] = fmaf(f, wmask_[c * 2 + j], o_m[j]);
#pragma unroll
            for (int t = 0; t < kTaps; ++t) o_a[t] = fmaf(f, wdna_[c * kTaps + t], o_a[t]);
        }
    }
}

// One output pixel (y, x) behind its head outputs: the two-way softmax (as composite_values: max, __expf, 1 / den), the
// pixel's kernel v_t = relu(a_t - shift) + shift, s = sum_t v_t (t ascending), g = mask_1 / s, ke_t = g * v_t, then
// of_c = mask_0 * prev_c and of_c = fma(ke_t, tap_t, of_c) with t ascending over the halo tile of composite_values
// (zero outside the image, fed-back distributions scaled by 1 / mass at the halo load); the distributions likewise; the
// cost terms of the CDNA path.
template <int ND, class PT>
__device__ __forceinline__ void composite_values_dna(const PT &p, const int y, const int x, float (&o_m)[2],
                                                     float (&o_a)[kTaps], const float *s_px, const int halo_w, const int hy,
                                                     const int hx, const int *goal, double (&cost)[2 * nd_slots(ND)], float (&of)[3],
                                                     float (&od)[nd_slots(ND)]) {
    constexpr int PS = comp_px_stride(ND);
    auto load_px = [&](const int sp, float (&fr)[3], float (&di)[nd_slots(ND)]) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(s_px + sp * PS);
        fr[0] = a[0]; fr[1] = a[1]; fr[2] = a[2];
        if constexpr (ND > 0) di[0] = a[3];
        if constexpr (ND > 1) {
            const f32x4 c2 = *reinterpret_cast<const f32x4 *>(s_px + sp * PS + 4);
#pragma unroll
            for (int d = 1; d < ND; ++d) di[d] = c2[d - 1];
        }
    };
    const float mx = fmaxf(o_m[0], o_m[1]);
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) { o_m[j] = __expf(o_m[j] - mx); den += o_m[j]; }
    const float inv = 1.0f / den;
#pragma unroll
    for (int j = 0; j < 2; ++j) o_m[j] *= inv;

    float s = 0.f;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) { o_a[t] = fmaxf(o_a[t] - kReluShift, 0.f) + kReluShift; s += o_a[t]; }
    const float g = o_m[1] / s;
    {
        float fr[3], di[nd_slots(ND)];
        load_px((hy + 2) * halo_w + (hx + 2), fr, di);
#pragma unroll
        for (int c = 0; c < 3; ++c) of[c] = o_m[0] * fr[c];
#pragma unroll
        for (int d = 0; d < ND; ++d) od[d] = o_m[0] * di[d];
    }
#pragma unroll
    for (int dy = 0; dy < kDnaKern; ++dy) {
#pragma unroll
        for (int dx = 0; dx < kDnaKern; ++dx) {
            const float ke = g * o_a[dy * kDnaKern + dx];
            float fr[3], di[nd_slots(ND)];
            load_px((hy + dy) * halo_w + (hx + dx), fr, di);
#pragma unroll
            for (int c = 0; c < 3; ++c) of[c] = fmaf(ke, fr[c], of[c]);
#pragma unroll
            for (int d = 0; d < ND; ++d) od[d] = fmaf(ke, di[d], od[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const float ry = (float)(y - goal[2 * d]), rx = (float)(x - goal[2 * d + 1]);
        const float dist = sqrtf(fmaf(ry, ry, rx * rx));
        cost[2 * d] = (double)od[d];
        cost[2 * d + 1] = (double)od[d] * (double)dist;
    }
}
// ... from the pixel's LDS feature row (the stand-alone tile and the fused top call this: same expressions, same bits)
template <int ND, class PT>
__device__ __forceinline__ void composite_pixel_values_dna(const PT &p, const int y, const int x, const float *feat,
                                                           const float mean, const float rstd, const float *s_px,
                                                           const int halo_w, const int hy, const int hx, const int *goal,
                                                           double (&cost)[2 * nd_slots(ND)], float (&of)[3], float (&od)[nd_slots(ND)]) {
    float o_m[2], o_a[kTaps];
    composite_dna_heads(p, feat, mean, rstd, o_m, o_a);
    composite_values_dna<ND>(p, y, x, o_m, o_a, s_px, halo_w, hy, hx, goal, cost, of, od);
}

// ------------------------------------------------------------------------------------------
// STP compositing (stp_arch.py; arXiv:1605.07157 section 3.3).  A two-layer FC head on the bottleneck
// predicts kStpWarps affine transforms per SAMPLE; warp k samples the whole previous frame and distributions at
//     xs = sx + t0 cx + t1 (sx / sy) cy + t2 sx,   ys = sy + t3 (sy / sx) cx + t4 cy + t5 sy
// (sx = (W - 1) / 2, sy = (H - 1) / 2, cx = x - sx, cy = y - sy) with the clamped bilinear taps of the flow path, and the
// masks mix the warps as they mix the flow path's.  The parameters are a per-sample table as the CDNA kernels are
// (PH_FC_PARTIAL + a finish item, CompositeParams::kern), the gathers reach any pixel as the flow path's do: the previous
// frame must be complete, which the dependency of the step's first conv on every compositing tile gives (emit_rollout).
constexpr int kStpWarps = 9;            // NF = num_masks - 1
constexpr int kStpHidden = 100;         // hidden units of the head (= 4 * kTaps: the first FC runs on the CDNA FC's plan)
constexpr int kStpRow = 6;              // floats per transform in global memory: [a0, a1, a2, b0, b1, b2]
constexpr int kStpRowPad = 8;           // ... and in LDS (two 16-byte reads per transform, every lane the same address)
static_assert(kStpWarps * kStpRowPad <= kTaps * kCompKernPad, "the transforms sit where the CDNA kernels sit in LDS");

// The finish item.  hid_j = relu(stp_fc/b_j + sum_split partial_j) (splits ascending, as cdna_finalize), theta_o = one fma
// chain over the hidden units ascending from stp/b_o, + the identity (1, 0, 0, 0, 1, 0), then the row in PIXEL units:
//     a0 = t0, a1 = t1 * (sx / sy), a2 = fma(t2, sx, sx);   b0 = t3 * (sy / sx), b1 = t4, b2 = fma(t5, sy, sy)
// so that a pixel computes xs = fma(a0, cx, fma(a1, cy, a2)), ys = fma(b0, cx, fma(b1, cy, b2)) (composite_values_stp).
// With theta the identity a2 = sx and xs = cx + sx = x exactly; with (-1, 0, 0, 0, -1, 0) xs = sx - cx = W - 1 - x exactly.
struct StpFinParams {
    const float *partial; int nsplit; int B;    // [nsplit][B][kStpHidden] raw sums of the first FC
    const float *bias;                          // stp_fc/b [kStpHidden]
    const float *w2, *b2;                       // stp/w [kStpHidden][kStpWarps * 6], stp/b [kStpWarps * 6]
    float *theta;                               // [B][kStpWarps][kStpRow], where the CDNA kernel table sits
    int H, W;
};

// one sample per workgroup call; scratch: kStpHidden floats of LDS
template <class PT>
__device__ __forceinline__ void stp_finalize_sample(const PT &p, const int b, float *scratch) {
    const int t = threadIdx.x;
    constexpr int NO = kStpWarps * kStpRow;
    if (t < kStpHidden) {
        float acc = p.bias[t];
        for (int z = 0; z < p.nsplit; ++z) acc += p.partial[((long long)z * p.B + b) * kStpHidden + t];
        scratch[t] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    if (t < NO) {
        float acc = p.b2[t];
        for (int j = 0; j < kStpHidden; ++j) acc = fmaf(scratch[j], p.w2[j * NO + t], acc);
        const int e = t % kStpRow;
        const float sx = 0.5f * (float)(p.W - 1), sy = 0.5f * (float)(p.H - 1);
        const float th = acc + ((e == 0 || e == 4) ? 1.0f : 0.0f);
        float v = th;
        if (e == 1) v = th * (sx / sy);
        else if (e == 2) v = fmaf(th, sx, sx);
        else if (e == 3) v = th * (sy / sx);
        else if (e == 5) v = fmaf(th, sy, sy);
        p.theta[(long long)b * NO + t] = v;
    }
}

// the per-layer launch of the finish item
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void stp_finalize_kernel(const StpFinParams p) {
    __shared__ float scratch[kStpHidden];
    stp_finalize_sample(p, blockIdx.x, scratch);
}

// One output pixel (y, x) behind its rgb / mask head outputs: softmax, nine affine warps, next frame / distributions, cost
// terms.  s_theta: the sample's transforms in LDS, [kStpWarps][kStpRowPad] in pixel units (above) - uniform over the
// workgroup, so they cost LDS broadcasts and no per-lane register beyond the row in use.  pf / pd / dscale, the clamp, the
// taps and the accumulation order are composite_values_flow's; there is no per-pixel head and no second pass over the
// feature row.
template <int ND, class PT>
__device__ __forceinline__ void composite_values_stp(const PT &p, const int y, const int x, float (&o_rgb)[3],
                                                     float (&o_m)[kStpWarps + 2], const float *s_theta, const float *pf,
                                                     const float *pd, const float *dscale, const int *goal,
                                                     double (&cost)[2 * nd_slots(ND)], float (&of)[3], float (&od)[nd_slots(ND)]) {
    constexpr int NM = kStpWarps + 2;
    float mx = o_m[0];
#pragma unroll
    for (int j = 1; j < NM; ++j) mx = fmaxf(mx, o_m[j]);
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < NM; ++j) { o_m[j] = __expf(o_m[j] - mx); den += o_m[j]; }
    const float inv = 1.0f / den;
#pragma unroll
    for (int j = 0; j < NM; ++j) o_m[j] *= inv;

    float sc[nd_slots(ND)];
#pragma unroll
    for (int d = 0; d < ND; ++d) sc[d] = dscale[d];
    {
        const long long o = (long long)y * p.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) of[c] = fmaf(o_m[0], pf[o * 3 + c], o_m[1] * sigmoidf_(o_rgb[c]));
#pragma unroll
        for (int d = 0; d < ND; ++d) od[d] = o_m[0] * (pd[o * ND + d] * sc[d]);
    }
    const float xmax = (float)(p.W - 1), ymax = (float)(p.H - 1);
    const float cx = (float)x - 0.5f * xmax, cy = (float)y - 0.5f * ymax;
#pragma unroll
    for (int k = 0; k < kStpWarps; ++k) {
        const f32x4 ta = *reinterpret_cast<const f32x4 *>(s_theta + k * kStpRowPad);
        const f32x4 tb = *reinterpret_cast<const f32x4 *>(s_theta + k * kStpRowPad + 4);
        const float xs = fmaf(ta[0], cx, fmaf(ta[1], cy, ta[2]));
        const float ys = fmaf(ta[3], cx, fmaf(tb[0], cy, tb[1]));
        // the taps of bilinear_clamped(), shared by the frame's channels and the distributions (a NaN clamps to 0)
        const float sx = fminf(fmaxf(xs, 0.f), xmax);
        const float sy = fminf(fmaxf(ys, 0.f), ymax);
        const int x0 = (int)floorf(sx), y0 = (int)floorf(sy);
        const int x1 = min(x0 + 1, p.W - 1), y1 = min(y0 + 1, p.H - 1);
        const float fx = sx - (float)x0, fy = sy - (float)y0;
        const int o00 = y0 * p.W + x0, o01 = y0 * p.W + x1, o10 = y1 * p.W + x0, o11 = y1 * p.W + x1;
        const float m = o_m[k + 2];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float a = pf[o00 * 3 + c], b = pf[o01 * 3 + c], cc = pf[o10 * 3 + c], dd = pf[o11 * 3 + c];
            const float top = fmaf(fx, b - a, a), bot = fmaf(fx, dd - cc, cc);
            of[c] = fmaf(m, fmaf(fy, bot - top, top), of[c]);
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            const float a = pd[o00 * ND + d] * sc[d], b = pd[o01 * ND + d] * sc[d];
            const float cc = pd[o10 * ND + d] * sc[d], dd = pd[o11 * ND + d] * sc[d];
            const float top = fmaf(fx, b - a, a), bot = fmaf(fx, dd - cc, cc);
            od[d] = fmaf(m, fmaf(fy, bot - top, top), od[d]);
        }
        // One warp's 4 x (3 + ND) gathers in flight at a time.  Every address of all nine warps is known up front (no
        // per-pixel head stands between them, as the flow path's does), and left alone the scheduler hoists the loads of
        // several warps: 226 VGPRs in the stand-alone tile, and spills in the fused top, which holds the conv tile's 64
        // accumulators across this function.
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        const float ry = (float)(y - goal[2 * d]), rx = (float)(x - goal[2 * d + 1]);
        const float dist = sqrtf(fmaf(ry, ry, rx * rx));
        cost[2 * d] = (double)od[d];
        cost[2 * d + 1] = (double)od[d] * (double)dist;
    }
}
// ... from the pixel's LDS feature row (the stand-alone tile and the fused top call this: same expressions, same bits)
template <int ND, class PT>
__device__ __forceinline__ void composite_pixel_values_stp(const PT &p, const int y, const int x, const float *feat,
                                                           const float mean, const float rstd, const float *s_theta,
                                                           const float *pf, const float *pd, const float *dscale,
                                                           const int *goal, double (&cost)[2 * nd_slots(ND)], float (&of)[3],
                                                           float (&od)[nd_slots(ND)]) {
    float o_rgb[3], o_m[kStpWarps + 2];
    composite_head_bias<kStpWarps + 1>(p, o_rgb, o_m);
    composite_heads<kStpWarps + 1>(p, feat, mean, rstd, 0, o_rgb, o_m);
    composite_values_stp<ND>(p, y, x, o_rgb, o_m, s_theta, pf, pd, dscale, goal, cost, of, od);
}

// compositing variants of composite_tile / fused_top_body / rollout_body (compile-time: the production kernel carries
// neither appearance-flow, DNA nor STP code and no run-time branch for them)
enum CompMode { COMP_CDNA = 0, COMP_FLOW = 1, COMP_DNA = 2, COMP_STP = 3 };

// one 16x16 pixel tile of one sample.  FIRST (arch 1, savp_arch.py): the first context frame is one more compositing
// layer - a template parameter, because a run-time branch around the mask bookkeeping costs the CDNA path 3.5 us per
// tile (measured).
// MODE COMP_FLOW (appearance flow, above): no halo tile and no kernel table are staged - the warps gather from global memory.
// MODE COMP_DNA (above): the halo tile is staged, the kernel table is not.
// MODE COMP_STP (above): no halo tile; the sample's nine transforms are staged where the kernel table sits.
template <int ND, int K, bool FIRST, class PT, int CFT = 32, int MODE = COMP_CDNA>
__device__ __forceinline__ void composite_tile(const PT &p, const int tile, const int b, const int *goal,
                                               float *smem) {
    constexpr int TS = kCompTile, HS = TS + 4;
    constexpr int NM = K + 1;
    constexpr int PS = comp_px_stride(ND);
    float *s_px = smem;                                 // [HS*HS][PS]: frame, distributions
    float *s_kern = s_px + HS * HS * PS;                // [kTaps][kCompKernPad]
    float *s_ln = s_kern + kTaps * kCompKernPad;        // [2]
    float *s_dscale = s_ln + 2;                         // [ND]
    float *s_enc = smem + ((composite_small_floats<ND, K>() + 3) & ~3);     // [TS*TS][kCompEncPad]

    const int tid = threadIdx.x;
    const int tilesX = (p.W + TS - 1) / TS;
    [[maybe_unused]] const int nblocks = sum_blocks(p.H, p.W);
    const int ty0 = (tile / tilesX) * TS, tx0 = (tile % tilesX) * TS;
    constexpr int CF = CFT;                     // feature channels per pixel (64: the public decoder table, two rounds below)

    // The tile's 32-channel features are fetched cooperatively - a wave instruction reads 1 KiB of consecutive
    // pixels - and transposed through LDS; one thread reading the 128 bytes of "its" pixel straight from memory
    // touches 64 cache lines per load instruction.  Issued first: the loads fly during the prologue below.
    f32x4 ev[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = tid + 256 * k, px = i >> 3, q = i & 7;
        const int yy = ty0 + (px >> 4), xx = tx0 + (px & 15);
        ev[k] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (yy < p.H && xx < p.W)
            ev[k] = *reinterpret_cast<const f32x4 *>(p.enc6 + (((long long)b * p.H + yy) * p.W + xx) * CF + q * 4);
    }

    // prologue reductions, lanes over the partials (32 LayerNorm partials and 64 tiles per sample at 128x128):
    // wave 0 the exact LayerNorm statistics, wave (d + 1) & 3 the mass of distribution d (fixed order: lanes
    // stride the tiles, then the xor butterfly - deterministic)
    {
        const int lane_ = tid & 63, wave_ = tid >> 6;
        if (wave_ == 0) {
            long long su = 0, sq = 0;
            const long long *pp = p.ln_part + (long long)b * p.ln_nparts * 2;
            for (int k = lane_; k < p.ln_nparts; k += 64) { su += pp[2 * k]; sq += pp[2 * k + 1]; }
            su = wave_sum(su); sq = wave_sum(sq);
            if (lane_ == 0) ln_from_totals(su, sq, p.ln_inv_n, s_ln[0], s_ln[1]);
        }
        for (int d = (wave_ + 3) & 3; d < ND; d += 4) {
            float sc = 1.0f;
            if (p.prev_sums) {
                double su = 0.0;
                const double *pp = p.prev_sums + ((long long)b * ND + d) * nblocks * 2;
                for (int k = lane_; k < nblocks; k += 64) su += pp[2 * k];
                su = wave_sum(su);
                sc = (float)(1.0 / su);
            }
            if (lane_ == 0) s_dscale[d] = sc;
        }
    }
    constexpr bool FLOW = MODE == COMP_FLOW, DNA = MODE == COMP_DNA, STP = MODE == COMP_STP;
    if constexpr (MODE == COMP_CDNA)
        for (int i = tid; i < kTaps * K; i += 256) s_kern[(i / K) * kCompKernPad + i % K] = p.kern[(long long)b * kTaps * K + i];
    if constexpr (STP)
        if (tid < kStpWarps * kStpRow)
            s_kern[(tid / kStpRow) * kStpRowPad + tid % kStpRow] = p.kern[(long long)b * (kStpWarps * kStpRow) + tid];
    __syncthreads();

    const float *pf = p.prev_frame + (long long)b * p.prev_frame_bstride;
    // (a frames-only tile, ND = 0: no distribution is staged, scaled or gathered; prev_distrib is null)
    const float *pd = ND > 0 ? p.prev_distrib + (long long)b * p.prev_distrib_bstride : nullptr;
    for (int i = tid; i < (FLOW || STP ? 0 : HS * HS); i += 256) {
        const int ly = i / HS, lx = i % HS;
        const int y = ty0 + ly - 2, x = tx0 + lx - 2;
        const bool in = y >= 0 && y < p.H && x >= 0 && x < p.W;
        const long long o = (long long)y * p.W + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) s_px[i * PS + c] = in ? pf[o * 3 + c] : 0.f;
#pragma unroll
        for (int d = 0; d < ND; ++d) s_px[i * PS + 3 + d] = in ? pd[o * ND + d] * s_dscale[d] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int i = tid + 256 * k;
        *reinterpret_cast<f32x4 *>(&s_enc[(i >> 3) * kCompEncPad + (i & 7) * 4]) = ev[k];
    }
    __syncthreads();

    const int ly = tid / TS, lx = tid % TS;
    const int y = ty0 + ly, x = tx0 + lx;
    const bool valid = y < p.H && x < p.W;
    double cost[2 * nd_slots(ND)];
#pragma unroll
    for (int i = 0; i < 2 * ND; ++i) cost[i] = 0.0;

    if constexpr (FLOW) {
        static_assert(!FLOW || (CF == 32 && K == kFlowWarps + 1 && !FIRST), "the flow table: survey decoder, ten masks");
        if (valid) {
            float of[3], od[nd_slots(ND)];
            composite_pixel_values_flow<ND>(p, y, x, &s_enc[tid * kCompEncPad], s_ln[0], s_ln[1], pf, pd, s_dscale, goal,
                                            cost, of, od);
            const long long o = (long long)y * p.W + x;
            float *fo = p.out_frame + (long long)b * p.out_frame_bstride + o * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) fo[c] = of[c];
            if constexpr (ND > 0) {
                float *dout = p.out_distrib + (long long)b * p.out_distrib_bstride + o * ND;
#pragma unroll
                for (int d = 0; d < ND; ++d) dout[d] = od[d];
            }
        }
    } else if constexpr (STP) {
        static_assert(!STP || (CF == 32 && K == kStpWarps + 1 && !FIRST), "the stp table: survey decoder, ten masks");
        if (valid) {
            float of[3], od[nd_slots(ND)];
            composite_pixel_values_stp<ND>(p, y, x, &s_enc[tid * kCompEncPad], s_ln[0], s_ln[1], s_kern, pf, pd, s_dscale,
                                           goal, cost, of, od);
            const long long o = (long long)y * p.W + x;
            float *fo = p.out_frame + (long long)b * p.out_frame_bstride + o * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) fo[c] = of[c];
            if constexpr (ND > 0) {
                float *dout = p.out_distrib + (long long)b * p.out_distrib_bstride + o * ND;
#pragma unroll
                for (int d = 0; d < ND; ++d) dout[d] = od[d];
            }
        }
    } else if constexpr (DNA) {
        static_assert(!DNA || (CF == 32 && K == 1 && !FIRST), "the dna table: survey decoder, one transform");
        if (valid) {
            float of[3], od[nd_slots(ND)];
            composite_pixel_values_dna<ND>(p, y, x, &s_enc[tid * kCompEncPad], s_ln[0], s_ln[1], s_px, HS, ly, lx, goal,
                                           cost, of, od);
            const long long o = (long long)y * p.W + x;
            float *fo = p.out_frame + (long long)b * p.out_frame_bstride + o * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) fo[c] = of[c];
            if constexpr (ND > 0) {
                float *dout = p.out_distrib + (long long)b * p.out_distrib_bstride + o * ND;
#pragma unroll
                for (int d = 0; d < ND; ++d) dout[d] = od[d];
            }
        }
    } else if constexpr (CF == 32) {
        if (valid)
            composite_pixel<ND, K, FIRST>(p, b, y, x, &s_enc[tid * kCompEncPad], s_ln[0], s_ln[1], s_px, s_kern, HS,
                                          ly, lx, goal, cost);
    } else {
        // 64 feature channels (cdna_arch.py decoder='public'): the heads accumulate over two 32-channel rounds through the
        // same LDS feature tile - channel order 0 .. 63, i.e. the fma chain of the one-round form continued
        float o_rgb[3], o_m[NM];
        composite_head_bias<K>(p, o_rgb, o_m);
        composite_heads<K>(p, &s_enc[tid * kCompEncPad], s_ln[0], s_ln[1], 0, o_rgb, o_m);     // (a pixel outside the image reads zeros)
#pragma unroll
        for (int c_off = 32; c_off < CF; c_off += 32) {
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int i = tid + 256 * k, px = i >> 3, q = i & 7;
                const int yy = ty0 + (px >> 4), xx = tx0 + (px & 15);
                f32x4 e = {0.f, 0.f, 0.f, 0.f};
                if (yy < p.H && xx < p.W)
                    e = *reinterpret_cast<const f32x4 *>(p.enc6 + (((long long)b * p.H + yy) * p.W + xx) * CF + c_off + q * 4);
                *reinterpret_cast<f32x4 *>(&s_enc[(i >> 3) * kCompEncPad + (i & 7) * 4]) = e;
            }
            __syncthreads();
            composite_heads<K>(p, &s_enc[tid * kCompEncPad], s_ln[0], s_ln[1], c_off, o_rgb, o_m);
        }
        if (valid) composite_finish<ND, K, FIRST>(p, b, y, x, o_rgb, o_m, s_px, s_kern, HS, ly, lx, goal, cost);
    }
    // ---- cost sums of this wave's block (4 rows x 16 columns): lanes in a fixed butterfly, one entry per block
    // (a frames-only tile has no cost terms and no out_sums)
    if constexpr (ND > 0) {
#pragma unroll
        for (int i = 0; i < 2 * ND; ++i) cost[i] = wave_sum(cost[i]);
        const int lane = tid & 63, wave = tid >> 6;
        const int by = ty0 / kSumBlockH + wave, bxk = tx0 / kSumBlockW;
        if (lane == 0 && by * kSumBlockH < p.H && tx0 < p.W) {
            const int blk = by * sum_blocks_x(p.W) + bxk;
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                double *dst = p.out_sums + (((long long)b * ND + d) * nblocks + blk) * 2;
                dst[0] = cost[2 * d]; dst[1] = cost[2 * d + 1];
            }
        }
    }
}

template <int ND, int K>
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void composite_kernel(const CompositeParams p) {
    __shared__ __attribute__((aligned(16))) float smem[composite_lds_floats<ND, K>()];
    if (K == 6 || p.first_frame) composite_tile<ND, K, true>(p, blockIdx.x, blockIdx.y, &p.goal[0][0], smem);
    else if constexpr (K != 6) {
        if (p.CF > 32) composite_tile<ND, K, false, CompositeParams, 64>(p, blockIdx.x, blockIdx.y, &p.goal[0][0], smem);
        else composite_tile<ND, K, false>(p, blockIdx.x, blockIdx.y, &p.goal[0][0], smem);
    }
}

// the per-layer launch of the appearance-flow compositing
template <int ND>
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void composite_flow_kernel(const CompositeParams p) {
    __shared__ __attribute__((aligned(16))) float smem[composite_lds_floats<ND, kFlowWarps + 1>()];
    composite_tile<ND, kFlowWarps + 1, false, CompositeParams, 32, COMP_FLOW>(p, blockIdx.x, blockIdx.y, &p.goal[0][0], smem);
}

// the per-layer launch of the DNA compositing
template <int ND>
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void composite_dna_kernel(const CompositeParams p) {
    __shared__ __attribute__((aligned(16))) float smem[composite_lds_floats<ND, 1>()];
    composite_tile<ND, 1, false, CompositeParams, 32, COMP_DNA>(p, blockIdx.x, blockIdx.y, &p.goal[0][0], smem);
}

// the per-layer launch of the STP compositing
template <int ND>
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void composite_stp_kernel(const CompositeParams p) {
    __shared__ __attribute__((aligned(16))) float smem[composite_lds_floats<ND, kStpWarps + 1>()];
    composite_tile<ND, kStpWarps + 1, false, CompositeParams, 32, COMP_STP>(p, blockIdx.x, blockIdx.y, &p.goal[0][0], smem);
}

// Frames-only engines (vf_config.ndesig = 0): the same tile with ND = 0 - no distribution halo, no scale of
// the previous distributions, no cost terms, no out_distrib / out_sums; a frame pixel runs the very fma chain of the ND = 1
// instance.  Kernels of their own NAME, not a fifth instance of the templates above: those are counted per designated-pixel
// count (tests/test_kernel_lint*.py).
template <int K>
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void composite_frames_kernel(const CompositeParams p) {
    __shared__ __attribute__((aligned(16))) float smem[composite_lds_floats<0, K>()];
    if (K == 6 || p.first_frame) composite_tile<0, K, true>(p, blockIdx.x, blockIdx.y, nullptr, smem);
    else if constexpr (K != 6) {
        if (p.CF > 32) composite_tile<0, K, false, CompositeParams, 64>(p, blockIdx.x, blockIdx.y, nullptr, smem);
        else composite_tile<0, K, false>(p, blockIdx.x, blockIdx.y, nullptr, smem);
    }
}
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void composite_flow_frames_kernel(const CompositeParams p) {
    __shared__ __attribute__((aligned(16))) float smem[composite_lds_floats<0, kFlowWarps + 1>()];
    composite_tile<0, kFlowWarps + 1, false, CompositeParams, 32, COMP_FLOW>(p, blockIdx.x, blockIdx.y, nullptr, smem);
}
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void composite_dna_frames_kernel(const CompositeParams p) {
    __shared__ __attribute__((aligned(16))) float smem[composite_lds_floats<0, 1>()];
    composite_tile<0, 1, false, CompositeParams, 32, COMP_DNA>(p, blockIdx.x, blockIdx.y, nullptr, smem);
}
VF_GLOBAL VF_LAUNCH_BOUNDS(256) void composite_stp_frames_kernel(const CompositeParams p) {
    __shared__ __attribute__((aligned(16))) float smem[composite_lds_floats<0, kStpWarps + 1>()];
    composite_tile<0, kStpWarps + 1, false, CompositeParams, 32, COMP_STP>(p, blockIdx.x, blockIdx.y, nullptr, smem);
}

// ------------------------------------------------------------------------------------------
// Cost finalisation.  Per rolled sequence r and task (view v, pixel d):
//     e[r][v*ND+d] = sum_t w_t (S1/S0)(t, v, r, d) / sum_t w_t,      w = (1, ..., 1, finalweight)
// (reference pixel_cost_controller.py:168-187); n_draws consecutive sequences are the latent draws
// of one action and are averaged; the action's score is the plain mean over tasks (reference :153)
// or, with use_weights, the trade-off weighted sum (register_gtruth_controller.py:88-94).
// Scores leave the device in float64 (the reference's host cost is float64 under NumPy >= 2,
// SURVEY section 7): no fp32 rounding can merge two distinct costs into a tie before the argsort.
// sums[t]: [ncam][Bcap][ND][blocks][2] (ntiles below = 4x16-pixel blocks per image).  A non-zero *status (a tile of the rollout gave up
// waiting for its producers) poisons every score with NaN, so a failed rollout cannot feed CEM.
constexpr int kMaxCam = 4;
struct TaskWeights { int use; float w[kMaxCam * kMaxDesig]; };

// One WAVE per action: the lanes stride the blocks of a (step, task, draw) and a fixed butterfly adds them up
// (deterministic; every reader of the sums uses this order).
VF_GLOBAL void scores_kernel(const double *sums, long long step_stride, long long view_stride, int n_actions,
                              int n_draws, int T, int ND, int ncam, int ntiles, float finalweight,
                              const TaskWeights tw, const int *status, double *scores, double *scores_per_task) {
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= n_actions) return;
    const int ntask = ncam * ND;
    const bool poisoned = status && *status != 0;
    double total = 0.0;
    for (int v = 0; v < ncam; ++v)
        for (int d = 0; d < ND; ++d) {
            double over_draws = 0.0;
            for (int j = 0; j < n_draws; ++j) {
                const long long b = (long long)a * n_draws + j;
                double acc = 0.0, wsum = 0.0;
                for (int t = 0; t < T; ++t) {
                    const double *pp = sums + (long long)t * step_stride + (long long)v * view_stride +
                                       (b * ND + d) * ntiles * 2;
                    double s0 = 0.0, s1 = 0.0;
                    for (int k = lane; k < ntiles; k += 64) { s0 += pp[2 * k]; s1 += pp[2 * k + 1]; }
                    s0 = wave_sum(s0); s1 = wave_sum(s1);
                    const double w = (t == T - 1) ? (double)finalweight : 1.0;
                    acc += w * (s1 / s0);
                    wsum += w;
                }
                over_draws += acc / wsum;
            }
            const double sc = over_draws / n_draws;
            const int col = v * ND + d;
            if (scores_per_task && lane == 0)
                scores_per_task[(long long)a * ntask + col] = poisoned ? __builtin_nan("") : sc;
            total += tw.use ? (double)tw.w[col] * sc : sc;
        }
    const double out = tw.use ? total : total / ntask;
    if (lane == 0) scores[a] = poisoned ? __builtin_nan("") : out;
}

// ------------------------------------------------------------------------------------------
// Ensemble cost (reference policy/cem_controllers/variants/ensemble_vidpred.py:32-61).  E engines of one config have
// rolled the same sequences; per (view v, pixel d, rolled sequence r, step t) member m's expected distance is
//     x_m = (S1/S0)_m(t, v, r, d)                         (the value that member's own scores_kernel used)
//     mean = sum_m x_m / E,  var = sum_m (x_m - mean)^2 / E   (two passes, population variance, members 0 .. E-1)
//     c_t = mean + lambda * var
// and c_t takes the place of S1/S0 in scores_kernel's reduction: time-weighted mean, mean over the action's draws,
// plain mean over tasks or the trade-off weighted sum.  The second pass re-reads the sums instead of holding E values
// per lane, so no member count costs registers or scratch.  cost_per_step (optional) [A][ncam*ND][T] gets c_t averaged
// over the draws.  A non-zero status of ANY member poisons every output with NaN.
constexpr int kMaxMembers = 16;
struct EnsembleMembers { const double *sums[kMaxMembers]; const int *status[kMaxMembers]; int n; };

__device__ __forceinline__ double member_step_cost(const double *pp, int ntiles, int lane) {
    double s0 = 0.0, s1 = 0.0;
    for (int k = lane; k < ntiles; k += 64) { s0 += pp[2 * k]; s1 += pp[2 * k + 1]; }
    s0 = wave_sum(s0); s1 = wave_sum(s1);
    return s1 / s0;
}

// One WAVE per action, as scores_kernel.
VF_GLOBAL void ensemble_scores_kernel(const EnsembleMembers em, long long step_stride, long long view_stride,
                                       int n_actions, int n_draws, int T, int ND, int ncam, int ntiles,
                                       float lambda_variance, float finalweight, const TaskWeights tw,
                                       double *scores, double *scores_per_task, double *cost_per_step) {
    const int a = blockIdx.x, lane = threadIdx.x;
    if (a >= n_actions) return;
    const int ntask = ncam * ND, E = em.n;
    bool poisoned = false;
    for (int m = 0; m < E; ++m) poisoned = poisoned || (em.status[m] && *em.status[m] != 0);
    const double lam = (double)lambda_variance;
    double total = 0.0;
    for (int v = 0; v < ncam; ++v)
        for (int d = 0; d < ND; ++d) {
            const int col = v * ND + d;
            double *cps = cost_per_step ? cost_per_step + ((long long)a * ntask + col) * T : nullptr;
            double over_draws = 0.0;
            for (int j = 0; j < n_draws; ++j) {
                const long long b = (long long)a * n_draws + j;
                const long long off0 = (long long)v * view_stride + (b * ND + d) * ntiles * 2;
                double acc = 0.0, wsum = 0.0;
                for (int t = 0; t < T; ++t) {
                    const long long off = (long long)t * step_stride + off0;
                    double sum = 0.0;
                    for (int m = 0; m < E; ++m) sum += member_step_cost(em.sums[m] + off, ntiles, lane);
                    const double mean = sum / (double)E;
                    double sq = 0.0;
                    for (int m = 0; m < E; ++m) {
                        const double dev = member_step_cost(em.sums[m] + off, ntiles, lane) - mean;
                        sq += dev * dev;
                    }
                    const double c = mean + lam * (sq / (double)E);
                    const double w = (t == T - 1) ? (double)finalweight : 1.0;
                    acc += w * c;
                    wsum += w;
                    if (cps && lane == 0) {     // (the same lane reads back what it wrote for the earlier draws)
                        const double s = j == 0 ? c : cps[t] + c;
                        cps[t] = poisoned ? __builtin_nan("") : (j == n_draws - 1 ? s / n_draws : s);
                    }
                }
                over_draws += acc / wsum;
            }
            const double sc = over_draws / n_draws;
            if (scores_per_task && lane == 0)
                scores_per_task[(long long)a * ntask + col] = poisoned ? __builtin_nan("") : sc;
            total += tw.use ? (double)tw.w[col] * sc : sc;
        }
    const double out = tw.use ? total : total / ntask;
    if (lane == 0) scores[a] = poisoned ? __builtin_nan("") : out;
}

// predictions out in the reference layout: dst[bb][t][view][hw][C] <- src[view][Bcap][t][hw][C]
// (reference vpred_model_interface.py:78,88 stacks the views on axis 2)
VF_GLOBAL void export_frames_kernel(const float *src, long long view_stride, int first, int count, int T,
                                     int ncam, int HWC, float *dst) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per_sample = (long long)T * ncam * HWC;
    if (i >= (long long)count * per_sample) return;
    const int bb = (int)(i / per_sample);
    const long long r = i - (long long)bb * per_sample;
    const int t = (int)(r / ((long long)ncam * HWC));
    const int v = (int)((r / HWC) % ncam);
    const int e = (int)(r % HWC);
    dst[i] = src[(long long)v * view_stride + ((long long)(first + bb) * T + t) * HWC + e];
}

// The normalisation every reader of a predicted distribution shares (vf_export, vf_render_plans): S0 of a plane is its
// block sums pp[2 * k] added in block order, a value leaves as (float)((double)src / S0).
__device__ __forceinline__ double distrib_s0(const double *pp, int ntiles) {
    double s0 = 0.0;
    for (int k = 0; k < ntiles; ++k) s0 += pp[2 * k];
    return s0;
}
__device__ __forceinline__ float distrib_normalised(float src, double s0) { return (float)((double)src / s0); }

// normalised distributions out: dst[bb][t][view][hw][d] = src[view][b][t][hw][d] / S0(t, view, b, d)
VF_GLOBAL void export_distrib_kernel(const float *src, long long view_stride, const double *sums,
                                      long long step_stride, long long sums_view_stride, int first, int count,
                                      int T, int ncam, int HW, int ND, int ntiles, float *dst) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per_sample = (long long)T * ncam * HW * ND;
    if (i >= (long long)count * per_sample) return;
    const int bb = (int)(i / per_sample);
    const long long r = i - (long long)bb * per_sample;
    const int t = (int)(r / ((long long)ncam * HW * ND));
    const int v = (int)((r / ((long long)HW * ND)) % ncam);
    const long long e = r % ((long long)HW * ND);
    const int d = (int)(e % ND);
    const int b = first + bb;
    const double *pp = sums + (long long)t * step_stride + (long long)v * sums_view_stride +
                       ((long long)b * ND + d) * ntiles * 2;
    dst[i] = distrib_normalised(src[(long long)v * view_stride + ((long long)b * T + t) * HW * ND + e],
                                distrib_s0(pp, ntiles));
}

// ------------------------------------------------------------------------------------------
// Grouped pixel cost (vf_group_pixel_scores): the expected distance of the resident, UNNORMALISED distributions of the last
// rollout to one goal per GROUP of rows (vf_set_contexts), where scores_kernel reduces the sums the rollout took against its
// one goal.  Per row b of group g = b / rows_per_group, view v, pixel d, step t:
//     S1 = sum over (r, c) of x[r][c] * sqrt((double)((r - gr)^2 + (c - gc)^2)),   (gr, gc) = goal[g][v][d]
// The squared distance is an exact integer, the root a float64 one, products and sums float64.  One workgroup per plane
// (b, v, t): thread k of 256 takes the pixel quads k, k + 256, ... in that order (a quad = 4 neighbours of one image row:
// W is a multiple of 8), the lanes of a wave add up in wave_sum's butterfly and the four waves in wave order.  That order
// depends on H and W alone, so a row's cost has the same bits in any batch, group count or position.  S0 is distrib_s0 of
// the plane's block sums - the divisor vf_export normalises with - and the plane's cost S1 / S0 goes to
// cost[b][v][d][t].  Traffic: ONE pass over the distributions, B * ncam * T * H * W * ND * 4 bytes in 16-byte loads - the
// kernel is bound by the memory system (HBM, or the last-level cache where the rollout's stores still sit), not by its
// float64 arithmetic (one root, one multiply and one add per value read).
constexpr int kGroupCostThreads = 256;
template <int ND>
VF_GLOBAL VF_LAUNCH_BOUNDS(kGroupCostThreads) void group_pixel_cost_kernel(
        const float *distrib, long long view_stride, const double *sums, long long step_stride, long long sums_view_stride,
        const int32_t *goal_pix, int rows_per_group, int NV, int T, int H, int W, int ntiles, double *cost) {
    __shared__ double s_part[kGroupCostThreads / 64][ND];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x % T, v = (blockIdx.x / T) % NV, b = blockIdx.x / (T * NV);
    const int g = b / rows_per_group;
    long long gr[ND], gc[ND];
    double acc[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        gr[d] = goal_pix[(((long long)g * NV + v) * ND + d) * 2];
        gc[d] = goal_pix[(((long long)g * NV + v) * ND + d) * 2 + 1];
        acc[d] = 0.0;
    }
    const long long HW = (long long)H * W;
    const f32x4 *src = reinterpret_cast<const f32x4 *>(distrib + (long long)v * view_stride + ((long long)b * T + t) * HW * ND);
    const int nquads = (int)(HW / 4);
    for (int k = tid; k < nquads; k += kGroupCostThreads) {
        float x[4 * ND];
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const f32x4 q = src[(long long)k * ND + i];
            x[4 * i] = q[0]; x[4 * i + 1] = q[1]; x[4 * i + 2] = q[2]; x[4 * i + 3] = q[3];
        }
        const int r = (4 * k) / W, c0 = (4 * k) % W;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const long long dr = r - gr[d], dc = c0 + q - gc[d];
                acc[d] += (double)x[q * ND + d] * sqrt((double)(dr * dr + dc * dc));
            }
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        acc[d] = wave_sum(acc[d]);
        if (lane == 0) s_part[wave][d] = acc[d];
    }
    __syncthreads();
    if (tid < ND) {
        double s1 = 0.0;
#pragma unroll
        for (int w = 0; w < kGroupCostThreads / 64; ++w) s1 += s_part[w][tid];
        const double *pp = sums + (long long)t * step_stride + (long long)v * sums_view_stride +
                           ((long long)b * ND + tid) * ntiles * 2;
        cost[(((long long)b * NV + v) * ND + tid) * T + t] = s1 / distrib_s0(pp, ntiles);
    }
}

// ... and scores_kernel's reduction of those plane costs, one thread per row: e = sum_t w_t cost / sum_t w_t with
// w = (1, ..., 1, finalweight), then the plain mean over tasks or the weighted sum with the weights of the row's GROUP.  The
// weights travel as a launch argument, kGroupWeightSets groups at a time: a launch scores the rows of the groups
// [gw.g0, gw.g0 + gw.n) (without weights one launch scores every row).  A raised *status poisons every output with NaN.
constexpr int kGroupWeightSets = 32;
struct GroupWeights { int use, g0, n; float w[kGroupWeightSets][kMaxCam * kMaxDesig]; };
VF_GLOBAL void group_scores_kernel(const double *cost, int B, int rows_per_group, int NV, int ND, int T, float finalweight,
                                    const GroupWeights gw, const int *status, double *scores, double *scores_per_task) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = gw.use ? gw.g0 * rows_per_group + i : i;
    const int b_end = gw.use ? min(B, (gw.g0 + gw.n) * rows_per_group) : B;
    if (b >= b_end) return;
    const int ntask = NV * ND, gl = gw.use ? b / rows_per_group - gw.g0 : 0;
    const bool poisoned = status && *status != 0;
    double total = 0.0;
    for (int col = 0; col < ntask; ++col) {
        const double *cp = cost + ((long long)b * ntask + col) * T;
        double acc = 0.0, wsum = 0.0;
        for (int t = 0; t < T; ++t) {
            const double w = (t == T - 1) ? (double)finalweight : 1.0;
            acc += w * cp[t];
            wsum += w;
        }
        const double sc = acc / wsum;
        if (scores_per_task) scores_per_task[(long long)b * ntask + col] = poisoned ? __builtin_nan("") : sc;
        total += gw.use ? (double)gw.w[gl][col] * sc : sc;
    }
    const double out = gw.use ? total : total / ntask;
    scores[b] = poisoned ? __builtin_nan("") : out;
}

// ------------------------------------------------------------------------------------------
// Registration (reference register_gtruth_controller.py:54-173).  A flow field (dx, dy) per
// reference pixel - the output of the registration network (vf_registration_net.h) - maps reference pixel
// (r, c) to the point (x, y) = (c + dx, r + dy) of the current frame ("warp_pts", :64-66).
__device__ __forceinline__ float bilinear_clamped(const float *img, int H, int W, float x, float y, int ch) {
    x = fminf(fmaxf(x, 0.f), (float)(W - 1));
    y = fminf(fmaxf(y, 0.f), (float)(H - 1));
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = x - (float)x0, fy = y - (float)y0;
    const float a = img[((long long)y0 * W + x0) * 3 + ch], b = img[((long long)y0 * W + x1) * 3 + ch];
    const float c = img[((long long)y1 * W + x0) * 3 + ch], d = img[((long long)y1 * W + x1) * 3 + ch];
    const float top = fmaf(fx, b - a, a), bot = fmaf(fx, d - c, c);
    return fmaf(fy, bot - top, top);
}

// warped[cam][r][c][:] = bilinear(current[cam], warp_pts[cam][r][c]);  pts[cam][r][c] = (x, y)
VF_GLOBAL void warp_image_kernel(const float *cur, const float *flow, int ncam, int H, int W, float *warped,
                                  float *pts) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncam * H * W) return;
    const int cam = i / (H * W), r = (i / W) % H, c = i % W;
    const float x = (float)c + flow[2 * i], y = (float)r + flow[2 * i + 1];
    if (pts) { pts[2 * i] = x; pts[2 * i + 1] = y; }
    if (warped)
        for (int ch = 0; ch < 3; ++ch)
            warped[3 * (long long)i + ch] = bilinear_clamped(cur + (long long)cam * H * W * 3, H, W, x, y, ch);
}

// One workgroup (128 threads) per (camera, task): re-localise the task's pixel and measure the
// warp error.  region == 0: the flow and the L2 photometric error at the pixel itself (:129-135,
// 163-170); region > 0: median flow and mean squared error over the (2*region+1)^2 window
// clipped to [0, size - clip_sub] (:139-161; the reference clips the start window with
// clip_sub = 1 and the goal window with 0).  desig = (row, col) float; an empty window gives NaN.
constexpr int kRegMaxWin = 11 * 11;
VF_GLOBAL VF_LAUNCH_BOUNDS(128) void register_kernel(const float *cur, const float *ref, const float *flow,
                                                       const int *pix, int ncam, int ntask, int H, int W,
                                                       int region, int clip_sub, float *desig, float *err) {
    __shared__ float s_x[kRegMaxWin], s_y[kRegMaxWin];
    __shared__ double s_red[2];
    __shared__ float s_med[4];
    const int cam = blockIdx.x / ntask, task = blockIdx.x % ntask, tid = threadIdx.x;
    const int pr = pix[(cam * ntask + task) * 2], pc = pix[(cam * ntask + task) * 2 + 1];
    const float *cur_c = cur + (long long)cam * H * W * 3, *ref_c = ref + (long long)cam * H * W * 3;
    const float *flow_c = flow + (long long)cam * H * W * 2;
    float *out_d = desig + (cam * ntask + task) * 2;
    if (region == 0) {
        if (tid == 0) {
            const int r = min(max(pr, 0), H - 1), c = min(max(pc, 0), W - 1);
            const float x = (float)c + flow_c[(r * W + c) * 2], y = (float)r + flow_c[(r * W + c) * 2 + 1];
            double acc = 0.0;
            for (int ch = 0; ch < 3; ++ch) {
                const float df = ref_c[(r * W + c) * 3 + ch] - bilinear_clamped(cur_c, H, W, x, y, ch);
                acc += (double)df * (double)df;
            }
            out_d[0] = y; out_d[1] = x;
            err[cam * ntask + task] = (float)sqrt(acc);
        }
        return;
    }
    const int hi_r = H - clip_sub, hi_c = W - clip_sub;
    const int r0 = min(max(pr - region, 0), hi_r), r1 = min(max(pr + region + 1, 0), hi_r);
    const int c0 = min(max(pc - region, 0), hi_c), c1 = min(max(pc + region + 1, 0), hi_c);
    const int wh = max(r1 - r0, 0), ww = max(c1 - c0, 0), n = wh * ww;
    if (n == 0) {
        if (tid == 0) { out_d[0] = out_d[1] = __builtin_nanf(""); err[cam * ntask + task] = __builtin_nanf(""); }
        return;
    }
    double sq = 0.0;
    if (tid < n) {
        const int r = r0 + tid / ww, c = c0 + tid % ww;
        const float x = (float)c + flow_c[(r * W + c) * 2], y = (float)r + flow_c[(r * W + c) * 2 + 1];
        s_x[tid] = x; s_y[tid] = y;
        for (int ch = 0; ch < 3; ++ch) {
            const float df = ref_c[(r * W + c) * 3 + ch] - bilinear_clamped(cur_c, H, W, x, y, ch);
            sq += (double)df * (double)df;
        }
    }
    sq = wave_sum(sq);
    if ((tid & 63) == 0) s_red[tid >> 6] = sq;
    __syncthreads();
    // medians by rank: element i has rank #{j : v_j < v_i or (v_j == v_i and j < i)}
    if (tid < n) {
        const float vx = s_x[tid], vy = s_y[tid];
        int rx = 0, ry = 0;
        for (int j = 0; j < n; ++j) {
            rx += (s_x[j] < vx) || (s_x[j] == vx && j < tid);
            ry += (s_y[j] < vy) || (s_y[j] == vy && j < tid);
        }
        const int lo = (n - 1) / 2, hi = n / 2;
        if (rx == lo) s_med[0] = vx;
        if (rx == hi) s_med[1] = vx;
        if (ry == lo) s_med[2] = vy;
        if (ry == hi) s_med[3] = vy;
    }
    __syncthreads();
    if (tid == 0) {
        out_d[0] = 0.5f * (s_med[2] + s_med[3]);        // row <- median y
        out_d[1] = 0.5f * (s_med[0] + s_med[1]);        // col <- median x
        err[cam * ntask + task] = (float)((s_red[0] + s_red[1]) / (double)(3 * n));
    }
}

}  // namespace vf
