// vf_frame_scorer.h - learned-cost planning: a small convolutional frame scorer (classifier / embedding head) run on the
// frames a rollout left in the engine, and the float64 cost reduction on top of it.  Replaces the host loop of the
// reference's visual_mpc/policy/cem_controllers/variants/classifier_controller.py:94-105 and nce_cost_controller.py:90-103
// (every predicted frame through control_embedding's network, then -log(p + 1e-5) resp. -<goal enc, frame enc>).
// Network: visual_foresight_amd/video_prediction/frame_scorer_arch.py (NHWC, float32; four 3x3 / 2 convolutions with zero
// padding 1, bias, ReLU: Cin -> 32 -> 64 -> 128 -> 128; mean over the positions; FC 128 -> D).
//
//   scorer_c1        vector ALU (K = 9 * Cin = 27 / 54): one workgroup per (frame, band of 8 output rows); the 17 input rows
//                    are staged in LDS with 16-byte loads straight from where the frame lies, scaled by input_scale;
//                    the weights sit beside them
//   scorer_conv      c2 - c4 on the matrix pipe: implicit GEMM, one wave per (frame, 32 output positions, NT * 32 output
//                    channels) tile, v_mfma_f32_32x32x2_f32 (exact fp32)
//   scorer_head      mean over the positions + FC, one workgroup per frame
//   scorer_raw_cost  float64: raw[b][t] = sum over views of -log(softmax(logits)[1] + 1e-5) resp. -<goal enc, enc>
//   scorer_scores    float64: time weighting (classifier_controller.py:135-142), mean over latent draws
//
// Same bits everywhere: every output value of every layer is ONE fmaf chain whose order depends on the layer alone -
//   c1:     (ky, kx, ci) ascending, then + bias;
//   c2..c4: the order of vf_net_conv.h (taps ascending, channels in steps of eight, K never split), then + bias;
//   gap:    positions in row-major order, then one division by their number;   fc: k ascending, then + bias.
// A frame's head output is therefore the same whatever batch, chunk, group, lane or rank it is scored in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vf_conv_mfma.h"
#include "vf_net_conv.h"

namespace vf {

constexpr int kScThreads = 256;
constexpr int kScBand = 8;              // output rows of c1 per workgroup (17 input rows staged)
constexpr int kScCh[5] = {0, 32, 64, 128, 128};     // output channels of c1 .. c4 ([0]: the tower's input channels)
constexpr int kScHeadThreads = 128;     // = kScCh[4]

// where the images of a pass lie: image (g, view c) starts at base + c * view_stride + (b * T + t) * img_stride with
// b = g / n_steps, t = t0 + g % n_steps.  Resident predictions: view_stride = max_batch * T * H * W * 3, img_stride =
// H * W * 3.  vf_scorer_embed's [n][ncam][H][W][Cin]: view_stride = H * W * Cin, img_stride = ncam * H * W * Cin, T = 1.
struct ScorerSrc {
    const float *base;
    long long view_stride, img_stride;
    int ncam, T, t0, n_steps;
};

// c1: out[fl][oy][ox][32] = relu(bias + sum_{ky, kx, ci} (scale * in[2 oy + ky - 1][2 ox + kx - 1][ci]) * w[ky][kx][ci][.]),
// fl = frame-view index inside the group (global index f0 + fl = g * ncam + c).  w / b: view c's at w + c * w_view_stride.
template <int CIN>
VF_GLOBAL VF_LAUNCH_BOUNDS(kScThreads) void
scorer_c1_kernel(ScorerSrc src, int f0, int H, int W, float scale, const float *__restrict__ w, const float *__restrict__ bias,
                 long long w_view_stride, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sc_rows[];         // [17][W * CIN] rows, then [9 * CIN][32] weights
    const int Ho = H / 2, Wo = W / 2, nbands = Ho / kScBand;
    const int fl = blockIdx.x / nbands, band = blockIdx.x % nbands;
    const int f = f0 + fl, c = f % src.ncam, g = f / src.ncam;
    const long long b = g / src.n_steps;
    const int t = src.t0 + g % src.n_steps;
    const float *img = src.base + (long long)c * src.view_stride + (b * src.T + t) * src.img_stride;
    const int row_f = W * CIN, row4 = row_f / 4;                            // (W a multiple of 16: whole 16-byte loads)
    const int iy0 = 2 * kScBand * band - 1;
    for (int i = threadIdx.x; i < (2 * kScBand + 1) * row4; i += kScThreads) {
        const int r = i / row4, q = i % row4, iy = iy0 + r;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (iy >= 0) {                                                      // (iy <= 16 band + 15 < H)
            v = reinterpret_cast<const float4 *>(img + (long long)iy * row_f)[q];
            v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        }
        reinterpret_cast<float4 *>(sc_rows)[i] = v;
    }
    // the view's weights next to the rows: every lane reads the same weight, an LDS broadcast (as scalar loads they fill
    // and overflow the scalar registers)
    float *sc_w = sc_rows + (2 * kScBand + 1) * row_f;
    for (int i = threadIdx.x; i < 9 * CIN * kScCh[1] / 4; i += kScThreads)
        reinterpret_cast<float4 *>(sc_w)[i] = reinterpret_cast<const float4 *>(w + c * w_view_stride)[i];
    __syncthreads();
    const float *wv = sc_w, *bv = bias + c * kScCh[1];
    for (int p = threadIdx.x; p < kScBand * Wo; p += kScThreads) {
        const int oyl = p / Wo, ox = p % Wo;
        float acc[kScCh[1]];
#pragma unroll
        for (int co = 0; co < kScCh[1]; ++co) acc[co] = 0.f;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {                                 // (a run-time loop: one tap's weights live at a time)
            const int ky = tap / 3, kx = tap % 3;
            const int ix = 2 * ox + kx - 1;                                 // (ix <= W - 1)
            const float *px = sc_rows + (2 * oyl + ky) * row_f + max(ix, 0) * CIN;
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) {
                const float x = ix >= 0 ? px[ci] : 0.f;
                const float *wk = wv + (tap * CIN + ci) * kScCh[1];
#pragma unroll
                for (int co = 0; co < kScCh[1]; ++co) acc[co] = fmaf(x, wk[co], acc[co]);
            }
        }
        float4 *o4 = reinterpret_cast<float4 *>(out + (((long long)fl * Ho + kScBand * band + oyl) * Wo + ox) * kScCh[1]);
#pragma unroll
        for (int q = 0; q < kScCh[1] / 4; ++q) {
            float4 v;
            v.x = fmaxf(acc[4 * q] + bv[4 * q], 0.f);         v.y = fmaxf(acc[4 * q + 1] + bv[4 * q + 1], 0.f);
            v.z = fmaxf(acc[4 * q + 2] + bv[4 * q + 2], 0.f); v.w = fmaxf(acc[4 * q + 3] + bv[4 * q + 3], 0.f);
            o4[q] = v;
        }
    }
}

// c2 .. c4: in [n][Hin][Win][Cin] -> out [n][Hin/2][Win/2][Cout], 3x3 / 2, zero padding 1, + bias, ReLU.  One wave per task =
// (frame fl, row tile of 32 output positions in row-major order, group of NT * 32 output channels); rows past the frame's
// last position are idle (not stored).  wp: packed by vf_scorer_load_weights in the layout of vf_net_conv.h.
template <int NT>
VF_GLOBAL VF_LAUNCH_BOUNDS(kNetConvThreads) void
scorer_conv_kernel(const float *__restrict__ in, int n_frames, int f0, int ncam, int Hin, int Win, int Cin, int Cout,
                   const float *__restrict__ wp, const float *__restrict__ bias, long long wp_view_stride,
                   float *__restrict__ out) {
    const int j = threadIdx.x & 31, half = (threadIdx.x & 63) >> 5;
    const int Wo = Win / 2, P = (Hin / 2) * Wo;
    int fl, mt, ng;
    if (!net_conv_task(n_frames, (P + 31) / 32, Cout / (32 * NT), fl, mt, ng)) return;
    const int c = (f0 + fl) % ncam;
    const int p = mt * 32 + j;

    f32x16 acc[NT];         // (stride 2: position (oy, ox) is centred on input (2 oy, 2 ox))
    net_conv3x3_mma<NT>(acc, in + (long long)fl * Hin * Win * Cin, Hin, Win, Cin, 2 * (p / Wo), 2 * (p % Wo), p < P,
                        reinterpret_cast<const f32x4 *>(wp + c * wp_view_stride), Cout / 32, ng, j, half);

    const float *bv = bias + c * Cout;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = (ng * NT + nt) * 32 + j;
        const float bc = bv[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int po = mt * 32 + net_mma_row(r, half);
            if (po < P) out[((long long)fl * P + po) * Cout + co] = fmaxf(acc[nt][r] + bc, 0.f);
        }
    }
}

// head: pooled[k] = (sum over the P positions of act[fl][p][k], p ascending) / P;  out[f0 + fl][d] = b[d] + sum_k pooled[k] *
// w[k][d], k ascending.  One workgroup of 128 threads per frame.
VF_GLOBAL VF_LAUNCH_BOUNDS(kScHeadThreads) void
scorer_head_kernel(const float *__restrict__ act, int f0, int ncam, int P, int D, const float *__restrict__ wfc,
                   const float *__restrict__ bfc, float *__restrict__ out) {
    __shared__ float pooled[kScCh[4]];
    const int fl = blockIdx.x, k = threadIdx.x, c = (f0 + fl) % ncam;
    const float *a = act + (long long)fl * P * kScCh[4] + k;
    float s = 0.f;
    for (int p = 0; p < P; ++p) s += a[(long long)p * kScCh[4]];
    pooled[k] = s / (float)P;
    __syncthreads();
    const float *wv = wfc + (long long)c * kScCh[4] * D, *bv = bfc + c * D;
    for (int d = k; d < D; d += kScHeadThreads) {
        float acc = 0.f;
        for (int i = 0; i < kScCh[4]; ++i) acc = fmaf(pooled[i], wv[(long long)i * D + d], acc);
        out[(long long)(f0 + fl) * D + d] = acc + bv[d];
    }
}

// raw[b * n_steps + s] = sum over views c (ascending) of x, from the head outputs enc [b][s][c][D] (float32):
//   head 0 (classifier): x = -log(p1 + 1e-5), p = softmax(logits) in float64          (classifier_controller.py:10,102-104)
//   head 1 (embedding):  x = -sum_d goal_enc[c][d] * enc[d], float64 products, d ascending  (nce_cost_controller.py:100-102,163)
VF_GLOBAL void scorer_raw_cost_kernel(const float *__restrict__ enc, const float *__restrict__ goal_enc, int n, int ncam, int D,
                                      int head, double *__restrict__ raw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double total = 0.0;
    for (int c = 0; c < ncam; ++c) {
        const float *e = enc + ((long long)i * ncam + c) * D;
        if (head == 0) {
            const double l0 = (double)e[0], l1 = (double)e[1], m = l0 > l1 ? l0 : l1;
            const double e0 = exp(l0 - m), e1 = exp(l1 - m);
            total += -log(e1 / (e0 + e1) + 1e-5);
        } else {
            const float *gq = goal_enc + (long long)c * D;
            double dot = 0.0;
            for (int d = 0; d < D; ++d) dot += (double)gq[d] * (double)e[d];
            total += -dot;
        }
    }
    raw[i] = total;
}

// Per action a (n_draws consecutive rolled sequences), classifier_controller.py:135-142 per sequence, then the mean over
// the draws in draw order:  finalweight >= 0 (n_steps == T): (sum_{t < T-1} raw_t + fw * raw_{T-1}) / (T - 1 + fw);
// finalweight < 0: raw of the last scored step.  cost_per_step (optional, n_steps == T) [A][T] = raw averaged over the draws.
// A non-zero *status turns every output into NaN, as scores_kernel does.
VF_GLOBAL void scorer_scores_kernel(const double *__restrict__ raw, int n_actions, int n_draws, int n_steps, float finalweight,
                                    const int *status, double *scores, double *cost_per_step) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_actions) return;
    const bool poisoned = status && *status != 0;
    const double nan = __builtin_nan(""), fw = (double)finalweight;
    double over_draws = 0.0;
    for (int jd = 0; jd < n_draws; ++jd) {
        const double *r = raw + ((long long)a * n_draws + jd) * n_steps;
        if (finalweight >= 0.f) {
            double acc = 0.0;
            for (int t = 0; t < n_steps - 1; ++t) acc += r[t];
            acc += fw * r[n_steps - 1];
            over_draws += acc / ((double)(n_steps - 1) + fw);
        } else {
            over_draws += r[n_steps - 1];
        }
    }
    scores[a] = poisoned ? nan : over_draws / n_draws;
    if (cost_per_step)
        for (int t = 0; t < n_steps; ++t) {
            double s = 0.0;
            for (int jd = 0; jd < n_draws; ++jd) s += raw[((long long)a * n_draws + jd) * n_steps + t];
            cost_per_step[(long long)a * n_steps + t] = poisoned ? nan : s / n_draws;
        }
}

// head outputs for the caller: a copy of enc, NaN under a raised status
VF_GLOBAL void scorer_copy_out_kernel(const float *__restrict__ enc, long long n, const int *status, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = (status && *status != 0) ? __builtin_nanf("") : enc[i];
}

}  // namespace vf
