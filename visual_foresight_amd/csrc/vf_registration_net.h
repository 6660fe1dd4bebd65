// vf_registration_net.h - the registration network on the device: the flow field that vf_register consumes, computed from
// the (current frame, reference image) pairs of a planning call.  Replaces the plug-in the reference builds with
// setup_gdn(gdnconf, gpu_id) (visual_mpc/policy/cem_controllers/register_gtruth_controller.py:7,21) and calls at :64-66.
// Network: visual_foresight_amd/video_prediction/registration_net_arch.py (NHWC, float32, m = ch_mult; three 3x3
// convolutions with ReLU and 2x2 max-pool 6 -> 32m -> 64m -> 128m, three 3x3 convolutions with ReLU and bilinear x2
// up-sampling 128m -> 64m -> 32m -> 16m, a 5x5 flow head 16m -> 2).
//
//   regnet_d1        vector ALU (K = 54): one workgroup per (image, band of 4 pooled rows, 32 output channels); the ten
//                    input rows of both images are staged in LDS with 16-byte loads, the weights sit beside them; ReLU
//                    and the 2x2 max-pool happen in registers
//   regnet_conv      d2, d3, u1, u2, u3 on the matrix pipe: implicit GEMM, stride 1, one wave per (image, tile of 32
//                    output positions = 32 / tw rows x tw columns, NT * 32 output channels), v_mfma_f32_32x32x2_f32
//                    (exact fp32); bias + ReLU in the epilogue; POOL: tw = 16, a lane holds whole 2x2 windows of its
//                    channel in its own accumulator registers and stores their maxima
//   regnet_upsample  per-channel four-tap bilinear transposed convolution (kernel 1 - |i - 1.5| / 2, stride 2, padding 1)
//   regnet_flow      vector ALU (two output channels, K = 25 * 16m): one thread per pixel
//
// Same bits everywhere: every output value of every layer is ONE fmaf chain whose order depends on the layer alone -
//   d1:        (ky, kx, ci) ascending with ci over concat[current, reference]; + bias; ReLU; max over the window;
//   d2 .. u3:  the order of vf_net_conv.h (taps ascending, channels in steps of eight, K never split); + bias; ReLU (and
//              the window maximum, which is exact, so max-then-bias equals bias-then-max);
//   up-sample: the (at most four) contributing inputs in (ky, kx) ascending order of the transposed-convolution kernel,
//              each an fmaf with the exactly representable weight k[ky] * k[kx];
//   flow:      (ky, kx, ci) ascending; + bias
// Padding taps multiply zeros or are skipped (fmaf(0, w, acc) == acc).  A pair's flow is therefore the same whatever call,
// slot or number of pairs it is computed with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vf_conv_mfma.h"
#include "vf_net_conv.h"

namespace vf {

constexpr int kRnThreads = 256;
constexpr int kRnBand = 4;              // pooled rows of d1 per workgroup (2 * 4 + 2 input rows staged)
constexpr int kRnFlowThreads = 64;
constexpr int kRnMaxSize = 128;         // height / width limit (registration_net_arch.MAX_SIZE)

// d1: out[img][py][px][co] = max over the 2x2 window of relu(bias + sum_{ky, kx, ci} x[y + ky - 1][x + kx - 1][ci] * w[ky][kx][ci][co]),
// x = concat[cur, ref].  img = pair * ncam + view; the view's weights [3][3][6][Cout] at w + view * 54 * Cout.
// grid: n_img * (H / 2 / kRnBand) * (Cout / 32)
VF_GLOBAL VF_LAUNCH_BOUNDS(kRnThreads) void
regnet_d1_kernel(const float *__restrict__ cur, const float *__restrict__ ref, int ncam, int H, int W, int Cout,
                 const float *__restrict__ w, const float *__restrict__ bias, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rn_rows[];     // [2][10][W * 3] rows, then [54][32] weights
    constexpr int kRows = 2 * kRnBand + 2;
    const int Ho = H / 2, Wo = W / 2, nbands = Ho / kRnBand, ngroups = Cout / 32;
    const int cg = blockIdx.x % ngroups, band = (blockIdx.x / ngroups) % nbands, img = blockIdx.x / (ngroups * nbands);
    const int c = img % ncam;
    const int row_f = W * 3, row4 = row_f / 4;                          // (W a multiple of 8: whole 16-byte loads)
    const int iy0 = 2 * kRnBand * band - 1;
    for (int i = threadIdx.x; i < 2 * kRows * row4; i += kRnThreads) {
        const int which = i / (kRows * row4), r = (i / row4) % kRows, q = i % row4, iy = iy0 + r;
        const float *src = (which ? ref : cur) + (long long)img * H * row_f;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (iy >= 0 && iy < H) v = reinterpret_cast<const float4 *>(src + (long long)iy * row_f)[q];
        reinterpret_cast<float4 *>(rn_rows)[i] = v;
    }
    float *rn_w = rn_rows + 2 * kRows * row_f;
    for (int i = threadIdx.x; i < 54 * 32; i += kRnThreads)
        rn_w[i] = w[(long long)c * 54 * Cout + (long long)(i / 32) * Cout + cg * 32 + (i % 32)];
    __syncthreads();
    const float *bv = bias + c * Cout + cg * 32;
    for (int p = threadIdx.x; p < kRnBand * Wo; p += kRnThreads) {
        const int pyl = p / Wo, px = p % Wo;
        float mx[32];
#pragma unroll
        for (int co = 0; co < 32; ++co) mx[co] = 0.f;                   // (ReLU: the maximum starts at zero)
#pragma unroll 1
        for (int win = 0; win < 4; ++win) {
            const int yl = 2 * pyl + (win >> 1), x = 2 * px + (win & 1);
            float acc[32];
#pragma unroll
            for (int co = 0; co < 32; ++co) acc[co] = 0.f;
#pragma unroll 1
            for (int tap = 0; tap < 9; ++tap) {                         // (a run-time loop: one tap's weights live at a time)
                const int ky = tap / 3, kx = tap % 3;
                const int ix = x + kx - 1;
                const bool ok = ix >= 0 && ix < W;
                const float *pc = rn_rows + (yl + ky) * row_f + (ok ? ix : 0) * 3;
#pragma unroll
                for (int ci = 0; ci < 6; ++ci) {
                    const float v = ok ? (ci < 3 ? pc[ci] : pc[kRows * row_f + ci - 3]) : 0.f;
                    const float *wk = rn_w + (tap * 6 + ci) * 32;
#pragma unroll
                    for (int co = 0; co < 32; ++co) acc[co] = fmaf(v, wk[co], acc[co]);
                }
            }
#pragma unroll
            for (int co = 0; co < 32; ++co) mx[co] = fmaxf(mx[co], acc[co] + bv[co]);
        }
        float4 *o4 = reinterpret_cast<float4 *>(out + (((long long)img * Ho + kRnBand * band + pyl) * Wo + px) * Cout + cg * 32);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float4 v = {mx[4 * q], mx[4 * q + 1], mx[4 * q + 2], mx[4 * q + 3]};
            o4[q] = v;
        }
    }
}

// d2 .. u3: in [n_img][Hin][Win][Cin] -> relu(conv 3x3 / 1, zero padding 1, + bias); POOL: the 2x2 maxima
// [n_img][Hin / 2][Win / 2][Cout], else [n_img][Hin][Win][Cout].  One wave per task = (image, tile of 32 / tw rows x tw
// columns, group of NT * 32 output channels), tw = 1 << tw_shift (16, or 8 for narrow maps; POOL needs 16 and even Hin, Win);
// positions past the map are idle (not stored).  wp: packed by vf_regnet_load_weights in the layout of vf_net_conv.h.
template <int NT, bool POOL>
VF_GLOBAL VF_LAUNCH_BOUNDS(kNetConvThreads) void
regnet_conv_kernel(const float *__restrict__ in, int n_img, int ncam, int Hin, int Win, int Cin, int Cout, int tw_shift,
                   const float *__restrict__ wp, const float *__restrict__ bias, long long wp_view_stride,
                   float *__restrict__ out) {
    const int j = threadIdx.x & 31, half = (threadIdx.x & 63) >> 5;
    const int tw = 1 << tw_shift, th = 32 >> tw_shift;
    const int tiles_x = (Win + tw - 1) >> tw_shift, tiles_y = (Hin + th - 1) / th;
    const int ntile_all = (Cout + 31) / 32;
    int img, mt, ng;
    if (!net_conv_task(n_img, tiles_x * tiles_y, ntile_all / NT, img, mt, ng)) return;
    const int c = img % ncam;
    const int y0 = (mt / tiles_x) * th, x0 = (mt % tiles_x) << tw_shift;
    const int y = y0 + (j >> tw_shift), x = x0 + (j & (tw - 1));

    f32x16 acc[NT];
    net_conv3x3_mma<NT>(acc, in + (long long)img * Hin * Win * Cin, Hin, Win, Cin, y, x, y < Hin && x < Win,
                        reinterpret_cast<const f32x4 *>(wp + c * wp_view_stride), ntile_all, ng, j, half);

    const float *bv = bias + c * Cout;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int co = (ng * NT + nt) * 32 + j;
        if (co >= Cout) continue;                                           // (u3 at m = 1: 16 channels in a 32-wide tile)
        const float bc = bv[co];
        if (POOL) {
            // tw = 16: tile row r, column cc is MFMA row 16 r + cc.  Lane half h holds the windows at columns
            // cc = 8 g + 4 h + 2 s (g, s in {0, 1}) in registers a, a + 1 (row 0) and a + 8, a + 9 (row 1), a = 2 s + 4 g.
            const int Ho = Hin / 2, Wo = Win / 2;
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const int a = 2 * s + 4 * g, xx = x0 + 8 * g + 4 * half + 2 * s;
                    const float m = fmaxf(fmaxf(acc[nt][a], acc[nt][a + 1]), fmaxf(acc[nt][a + 8], acc[nt][a + 9]));
                    if (xx < Win && y0 < Hin)
                        out[(((long long)img * Ho + y0 / 2) * Wo + xx / 2) * Cout + co] = fmaxf(m + bc, 0.f);
                }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = net_mma_row(r, half);
                const int yy = y0 + (i >> tw_shift), xx = x0 + (i & (tw - 1));
                if (yy < Hin && xx < Win) out[(((long long)img * Hin + yy) * Win + xx) * Cout + co] = fmaxf(acc[nt][r] + bc, 0.f);
            }
        }
    }
}

// up-sampling: in [n_img][h][w][C] -> out [n_img][2 h][2 w][C], out[o] = sum_i in[i] * k[o - 2 i + 1] per axis, k = (0.25,
// 0.75, 0.75, 0.25) (savp3's bilinear transposed convolution).  An output row takes k[1] of row o / 2 and k[3] of row
// o / 2 - 1 when o is even, k[0] of row (o + 1) / 2 and k[2] of row (o - 1) / 2 when odd.  One thread per four channels.
VF_GLOBAL VF_LAUNCH_BOUNDS(kRnThreads) void
regnet_upsample_kernel(const float *__restrict__ in, long long n_out4, int h, int w, int C, float *__restrict__ out) {
    const long long i = (long long)blockIdx.x * kRnThreads + threadIdx.x;
    if (i >= n_out4) return;
    const int C4 = C / 4;
    const int c4 = (int)(i % C4), ox = (int)((i / C4) % (2 * w)), oy = (int)((i / ((long long)C4 * 2 * w)) % (2 * h));
    const long long img = i / ((long long)C4 * 2 * w * 2 * h);
    const float4 *src = reinterpret_cast<const float4 *>(in + img * h * w * C) + c4;
    // the two taps of an axis in ascending kernel index: (input index, weight)
    const int ya = (oy & 1) ? (oy + 1) / 2 : oy / 2, yb = (oy & 1) ? (oy - 1) / 2 : oy / 2 - 1;
    const int xa = (ox & 1) ? (ox + 1) / 2 : ox / 2, xb = (ox & 1) ? (ox - 1) / 2 : ox / 2 - 1;
    const float wya = (oy & 1) ? 0.25f : 0.75f, wyb = (oy & 1) ? 0.75f : 0.25f;
    const float wxa = (ox & 1) ? 0.25f : 0.75f, wxb = (ox & 1) ? 0.75f : 0.25f;
    float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int iy = (t >> 1) ? yb : ya, ix = (t & 1) ? xb : xa;
        const float wt = ((t >> 1) ? wyb : wya) * ((t & 1) ? wxb : wxa);
        if (iy >= 0 && iy < h && ix >= 0 && ix < w) {
            const float4 v = src[((long long)iy * w + ix) * C4];
            acc.x = fmaf(v.x, wt, acc.x); acc.y = fmaf(v.y, wt, acc.y);
            acc.z = fmaf(v.z, wt, acc.z); acc.w = fmaf(v.w, wt, acc.w);
        }
    }
    reinterpret_cast<float4 *>(out)[i] = acc;
}

// flow head: out[img][y][x][d] = bias[d] + sum_{ky, kx, ci} in[y + ky - 2][x + kx - 2][ci] * w[ky][kx][ci][d], d = 0, 1.
// One thread per pixel (H * W is a multiple of 64: a workgroup stays inside one image); the view's weights in LDS.
VF_GLOBAL VF_LAUNCH_BOUNDS(kRnFlowThreads) void
regnet_flow_kernel(const float *__restrict__ in, int ncam, int H, int W, int Cin, const float *__restrict__ w,
                   const float *__restrict__ bias, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float rn_fw[];           // [25][Cin][2]
    const long long pix = (long long)blockIdx.x * kRnFlowThreads + threadIdx.x;
    const int img = (int)(pix / ((long long)H * W)), c = img % ncam;
    const int y = (int)((pix / W) % H), x = (int)(pix % W);
    const int nw = 25 * Cin * 2;
    for (int i = threadIdx.x; i < nw; i += kRnFlowThreads) rn_fw[i] = w[(long long)c * nw + i];
    __syncthreads();
    const float *src = in + (long long)img * H * W * Cin;
    float a0 = 0.f, a1 = 0.f;
    for (int tap = 0; tap < 25; ++tap) {
        const int iy = y + tap / 5 - 2, ix = x + tap % 5 - 2;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        const float4 *p4 = reinterpret_cast<const float4 *>(src + ((long long)iy * W + ix) * Cin);
        const float2 *w2 = reinterpret_cast<const float2 *>(rn_fw) + tap * Cin;
        for (int q = 0; q < Cin / 4; ++q) {
            const float4 v = p4[q];
            const float2 w0 = w2[4 * q], w1 = w2[4 * q + 1], wv2 = w2[4 * q + 2], w3 = w2[4 * q + 3];
            a0 = fmaf(v.x, w0.x, a0);  a1 = fmaf(v.x, w0.y, a1);
            a0 = fmaf(v.y, w1.x, a0);  a1 = fmaf(v.y, w1.y, a1);
            a0 = fmaf(v.z, wv2.x, a0); a1 = fmaf(v.z, wv2.y, a1);
            a0 = fmaf(v.w, w3.x, a0);  a1 = fmaf(v.w, w3.y, a1);
        }
    }
    float2 o = {a0 + bias[c * 2], a1 + bias[c * 2 + 1]};
    reinterpret_cast<float2 *>(out)[pix] = o;
}

}  // namespace vf
