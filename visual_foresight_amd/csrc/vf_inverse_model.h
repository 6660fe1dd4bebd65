// vf_inverse_model.h - the action-inference network of the inverse-model policy on the device: from (start image, goal
// image, context frames, context actions) to the next n_actions actions without leaving the device.  Replaces the
// predictor the reference builds from robonet.inverse_model.testing.action_inference_interface
// (visual_mpc/policy/inverse_models/inverse_model_base_controller.py:4,31-32) and calls at :79-80.
// Network: visual_foresight_amd/video_prediction/inverse_model_arch.py (NHWC, float32; two towers of the frame scorer's
// convolution table - `pair` on concat[goal, start], `ctx` on every context frame - with a mean over the positions, and
// an LSTM cell of 128 units that is warmed up on the context and then decodes the actions).
//
// A call with n problems has n * (1 + n_context) images: image g < n is problem g's (goal, start) pair, image
// n + g * n_context + i is context frame i of problem g.  Every layer runs all of them in ONE launch; a workgroup (c1) or
// a wave (c2 .. c4) picks its tower's weights by its image index.  Six launches per call, whatever n_actions is:
//
//   invmodel_c1      vector ALU (K = 54 / 27): one workgroup per (image, band of 8 output rows); the 17 input rows are
//                    staged in LDS, scaled by input_scale - the pair tower stages goal and start from their own buffers
//                    (no concatenated copy exists); the weights sit beside them
//   invmodel_conv    c2 - c4 on the matrix pipe through vf_net_conv.h, one wave per (image, 32 positions, NT * 32 channels)
//   invmodel_gates   one workgroup per image: the mean over the positions (128 threads), then the input part of the gate
//                    sums b + x Wx for all 512 gate rows - once per feature vector, so p's product is not repeated in
//                    the decode steps
//   invmodel_lstm    the whole recurrence, n_context + n_actions steps, in one launch: one workgroup of 512 threads per
//                    problem, thread r owns gate row r (gates i, f, g, o x 128 units) and keeps its column of Wh (128
//                    values) and of Wa in registers for every step (fp32 Wh is 256 KiB: more than the 160 KiB of LDS, but
//                    512 x 128 registers hold it; two waves per SIMD leave 256 registers a lane); Wo and bo live in LDS; h
//                    and the fed-back action travel through LDS between the steps.  Three workgroup barriers a step (gate
//                    sums -> cell update -> action), no cross-workgroup synchronisation of any kind
//
// Same bits everywhere: every value is ONE fmaf chain whose order depends on the layer alone -
//   c1:      (ky, kx, ci) ascending with ci over concat[goal, start]; then + bias;
//   c2..c4:  the order of vf_net_conv.h; then + bias;
//   pool:    positions in row-major order, then one division by their number;
//   gates:   z = b, then x[k] Wx[k] for k ascending (invmodel_gates), then a[k] Wa[k] for k ascending, then h[k] Wh[k] for k
//            ascending (invmodel_lstm);  c' = sigmoid(f) * c + sigmoid(i) * tanh(g), h' = sigmoid(o) * tanh(c') with
//            sigmoid(v) = 1 / (1 + expf(-v)), two roundings per product-sum (the library is built without contraction);
//   action:  h[k] Wo[k] for k ascending from zero, then + bo.
// A problem's actions are therefore the same whatever n, slot or call they are computed in, and the first actions do not
// depend on n_actions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vf_conv_mfma.h"
#include "vf_net_conv.h"
#include "vf_frame_scorer.h"

namespace vf {

constexpr int kImThreads = 256;         // c1
constexpr int kImBand = kScBand;        // output rows of c1 per workgroup (17 input rows staged)
constexpr int kImUnits = 128;           // LSTM width = kScCh[4]
constexpr int kImGates = 4 * kImUnits;  // gate rows = threads of invmodel_gates / invmodel_lstm
constexpr int kImMaxAdim = 8;
constexpr int kImMaxContext = 4;

// where the images of a call lie (all float32 NHWC, 3 channels, 16-byte aligned)
struct InvModelSrc {
    const float *start, *goal;          // [n][H][W][3]
    const float *ctx;                   // [n][n_context][H][W][3]
    int n, n_context;
};

// one band of c1 for one image with NSRC sources of three channels each (channel ci of the layer = source ci / 3)
template <int NSRC>
__device__ __forceinline__ void invmodel_c1_band(float *rows, const float *src0, const float *src1, int band, int H, int W,
                                                 float scale, const float *__restrict__ w, const float *__restrict__ bias,
                                                 float *__restrict__ out_img) {
    constexpr int CIN = 3 * NSRC, kRows = 2 * kImBand + 1;
    const int Wo = W / 2;
    const int row_f = W * 3, row4 = row_f / 4;                              // (W a multiple of 16: whole 16-byte loads)
    const int iy0 = 2 * kImBand * band - 1;
    for (int i = threadIdx.x; i < NSRC * kRows * row4; i += kImThreads) {
        const int which = i / (kRows * row4), r = (i / row4) % kRows, q = i % row4, iy = iy0 + r;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (iy >= 0) {                                                      // (iy <= 16 band + 15 < H)
            v = reinterpret_cast<const float4 *>((which ? src1 : src0) + (long long)iy * row_f)[q];
            v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
        }
        reinterpret_cast<float4 *>(rows)[i] = v;
    }
    float *sw = rows + 2 * kRows * row_f;                                   // (behind the rows of the wider tower)
    for (int i = threadIdx.x; i < 9 * CIN * kScCh[1] / 4; i += kImThreads)
        reinterpret_cast<float4 *>(sw)[i] = reinterpret_cast<const float4 *>(w)[i];
    __syncthreads();
    for (int p = threadIdx.x; p < kImBand * Wo; p += kImThreads) {
        const int oyl = p / Wo, ox = p % Wo;
        float acc[kScCh[1]];
#pragma unroll
        for (int co = 0; co < kScCh[1]; ++co) acc[co] = 0.f;
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {                                 // (a run-time loop: one tap's weights live at a time)
            const int ky = tap / 3, kx = tap % 3;
            const int ix = 2 * ox + kx - 1;                                 // (-1 <= ix <= W - 1)
            const float *px = rows + (2 * oyl + ky) * row_f + max(ix, 0) * 3;
#pragma unroll
            for (int ci = 0; ci < CIN; ++ci) {
                const float x = ix >= 0 ? px[(ci / 3) * kRows * row_f + ci % 3] : 0.f;
                const float *wk = sw + (tap * CIN + ci) * kScCh[1];
#pragma unroll
                for (int co = 0; co < kScCh[1]; ++co) acc[co] = fmaf(x, wk[co], acc[co]);
            }
        }
        float4 *o4 = reinterpret_cast<float4 *>(out_img + ((long long)(kImBand * band + oyl) * Wo + ox) * kScCh[1]);
#pragma unroll
        for (int q = 0; q < kScCh[1] / 4; ++q) {
            float4 v;
            v.x = fmaxf(acc[4 * q] + bias[4 * q], 0.f);         v.y = fmaxf(acc[4 * q + 1] + bias[4 * q + 1], 0.f);
            v.z = fmaxf(acc[4 * q + 2] + bias[4 * q + 2], 0.f); v.w = fmaxf(acc[4 * q + 3] + bias[4 * q + 3], 0.f);
            o4[q] = v;
        }
    }
}

// c1 of both towers: out[img][oy][ox][32] = relu(bias + sum_{ky, kx, ci} (scale * in[2 oy + ky - 1][2 ox + kx - 1][ci]) * w[ky][kx][ci][.])
// grid: n * (1 + n_context) * (H / 2 / kImBand); dynamic LDS: (2 * 17 * W * 3 + 9 * 6 * 32) floats
VF_GLOBAL VF_LAUNCH_BOUNDS(kImThreads) void
invmodel_c1_kernel(InvModelSrc src, int H, int W, float scale, const float *__restrict__ w_pair, const float *__restrict__ b_pair,
                   const float *__restrict__ w_ctx, const float *__restrict__ b_ctx, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float im_rows[];
    const int nbands = H / 2 / kImBand;
    const int img = blockIdx.x / nbands, band = blockIdx.x % nbands;
    const long long frame = (long long)H * W * 3;
    float *out_img = out + (long long)img * (H / 2) * (W / 2) * kScCh[1];
    if (img < src.n)                    // (uniform over the workgroup)
        invmodel_c1_band<2>(im_rows, src.goal + img * frame, src.start + img * frame, band, H, W, scale, w_pair, b_pair, out_img);
    else
        invmodel_c1_band<1>(im_rows, src.ctx + (img - src.n) * frame, nullptr, band, H, W, scale, w_ctx, b_ctx, out_img);
}

// c2 .. c4 of both towers: in [n_img][Hin][Win][Cin] -> out [n_img][Hin/2][Win/2][Cout], 3x3 / 2, zero padding 1, + bias,
// ReLU.  One wave per task (vf_net_conv.h); images below n_pair take the first weight set of wp [2][packed] / bias [2][Cout].
template <int NT>
VF_GLOBAL VF_LAUNCH_BOUNDS(kNetConvThreads) void
invmodel_conv_kernel(const float *__restrict__ in, int n_img, int n_pair, int Hin, int Win, int Cin, int Cout,
                     const float *__restrict__ wp, const float *__restrict__ bias, long long wp_tower_stride,
                     float *__restrict__ out) {
    const int j = threadIdx.x & 31, half = (threadIdx.x & 63) >> 5;
    const int Wo = Win / 2, P = (Hin / 2) * Wo;
    int img, mt, ng;
    if (!net_conv_task(n_img, (P + 31) / 32, Cout / (32 * NT), img, mt, ng)) return;
    const int tw = img < n_pair ? 0 : 1;
    const int p = mt * 32 + j;

    f32x16 acc[NT];         // (stride 2: position (oy, ox) is centred on input (2 oy, 2 ox))
    net_conv3x3_mma<NT>(acc, in + (long long)img * Hin * Win * Cin, Hin, Win, Cin, 2 * (p / Wo), 2 * (p % Wo), p < P,
                        reinterpret_cast<const f32x4 *>(wp + tw * wp_tower_stride), Cout / 32, ng, j, half);

    const float *bv = bias + tw * Cout;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = (ng * NT + nt) * 32 + j;
        const float bc = bv[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int po = mt * 32 + net_mma_row(r, half);
            if (po < P) out[((long long)img * P + po) * Cout + co] = fmaxf(acc[nt][r] + bc, 0.f);
        }
    }
}

// pooled[k] = (sum over the P positions of act[img][p][k], p ascending) / P;  pre[img][r] = b[r] + sum_k pooled[k] * wx[k][r],
// k ascending from b.  One workgroup of 512 threads per image; wx [128][512].
VF_GLOBAL VF_LAUNCH_BOUNDS(kImGates) void
invmodel_gates_kernel(const float *__restrict__ act, int P, const float *__restrict__ wx, const float *__restrict__ b,
                      float *__restrict__ pre) {
    __shared__ float pooled[kImUnits];
    const int img = blockIdx.x, r = threadIdx.x;
    if (r < kImUnits) {
        const float *a = act + (long long)img * P * kImUnits + r;
        float s = 0.f;
        for (int p = 0; p < P; ++p) s += a[(long long)p * kImUnits];
        pooled[r] = s / (float)P;
    }
    __syncthreads();
    float acc = b[r];
#pragma unroll 8
    for (int k = 0; k < kImUnits; ++k) acc = fmaf(pooled[k], wx[k * kImGates + r], acc);
    pre[(long long)img * kImGates + r] = acc;
}

// the LDS traffic of a step is complete before the workgroup meets (tools/lint_barriers.py: hipcc does not wait for an
// LDS store that is pending on a loop's back edge in front of a loop-head barrier; the wait is explicit)
__device__ __forceinline__ void invmodel_step_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

__device__ __forceinline__ float invmodel_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// The recurrence of problem blockIdx.x: n_context warm-up steps (x = q_i, a = context action i), then n_actions decode
// steps (x = p, a = the previous action; the last context action at first).  pre [n * (1 + n_context)][512] are the input
// parts of the gate sums in the image order of the call; wa [adim][512], wh [128][512], wo [128][adim], bo [adim].
// actions [n][n_actions][adim]; hidden (optional) [n][n_context + n_actions][2][128] = h, c after every step.
VF_GLOBAL VF_LAUNCH_BOUNDS(kImGates) void
invmodel_lstm_kernel(const float *__restrict__ pre, const float *__restrict__ ctx_actions, int n, int adim, int n_context,
                     int n_actions, const float *__restrict__ wa, const float *__restrict__ wh, const float *__restrict__ wo,
                     const float *__restrict__ bo, float *__restrict__ actions, float *__restrict__ hidden) {
    __shared__ __attribute__((aligned(16))) float sh_h[kImUnits];
    __shared__ float sh_z[kImGates];
    __shared__ float sh_a[kImMaxAdim];                          // the action fed back
    __shared__ float sh_ca[kImMaxContext * kImMaxAdim];         // the context actions
    __shared__ float sh_wo[kImUnits * kImMaxAdim];
    __shared__ float sh_bo[kImMaxAdim];
    const int r = threadIdx.x, prob = blockIdx.x;

    float whr[kImUnits];                                        // column r of Wh, on the chip for every step
#pragma unroll
    for (int k = 0; k < kImUnits; ++k) whr[k] = wh[k * kImGates + r];
    float war[kImMaxAdim];
#pragma unroll
    for (int k = 0; k < kImMaxAdim; ++k) war[k] = k < adim ? wa[k * kImGates + r] : 0.f;
    for (int i = r; i < kImUnits * adim; i += kImGates) sh_wo[i] = wo[i];
    if (r < adim) sh_bo[r] = bo[r];
    if (r < n_context * adim) sh_ca[(r / adim) * kImMaxAdim + r % adim] = ctx_actions[(long long)prob * n_context * adim + r];
    if (r < kImUnits) sh_h[r] = 0.f;
    float c = 0.f;                                              // unit r's cell state (threads below 128)
    const float pre_p = pre[(long long)prob * kImGates + r];    // b + p Wx: the same in every decode step
    invmodel_step_barrier();

    const int steps = n_context + n_actions;
    for (int s = 0; s < steps; ++s) {
        const bool warm = s < n_context;
        float acc = warm ? pre[((long long)n + (long long)prob * n_context + s) * kImGates + r] : pre_p;
        const float *av = warm ? sh_ca + s * kImMaxAdim : (s == n_context ? sh_ca + (n_context - 1) * kImMaxAdim : sh_a);
#pragma unroll
        for (int k = 0; k < kImMaxAdim; ++k)
            if (k < adim) acc = fmaf(av[k], war[k], acc);
#pragma unroll
        for (int q = 0; q < kImUnits / 4; ++q) {
            const float4 hv = reinterpret_cast<const float4 *>(sh_h)[q];        // (an LDS broadcast)
            acc = fmaf(hv.x, whr[4 * q], acc);
            acc = fmaf(hv.y, whr[4 * q + 1], acc);
            acc = fmaf(hv.z, whr[4 * q + 2], acc);
            acc = fmaf(hv.w, whr[4 * q + 3], acc);
        }
        sh_z[r] = acc;
        invmodel_step_barrier();                                // every gate sum of the step is in LDS; sh_h has been read
        if (r < kImUnits) {
            const float gi = invmodel_sigmoid(sh_z[r]), gf = invmodel_sigmoid(sh_z[kImUnits + r]);
            const float gg = tanhf(sh_z[2 * kImUnits + r]), go = invmodel_sigmoid(sh_z[3 * kImUnits + r]);
            c = gf * c + gi * gg;
            const float h = go * tanhf(c);
            sh_h[r] = h;
            if (hidden) {
                float *hc = hidden + ((long long)prob * steps + s) * 2 * kImUnits;
                hc[r] = h;
                hc[kImUnits + r] = c;
            }
        }
        invmodel_step_barrier();                                // the new h is in LDS; sh_z has been read
        if (!warm) {                                            // (uniform over the workgroup)
            if (r < adim) {
                float a = 0.f;
                for (int k = 0; k < kImUnits; ++k) a = fmaf(sh_h[k], sh_wo[k * adim + r], a);
                a += sh_bo[r];
                sh_a[r] = a;
                actions[((long long)prob * n_actions + (s - n_context)) * adim + r] = a;
            }
            invmodel_step_barrier();                            // the action is in LDS for the next step
        }
    }
}

}  // namespace vf
