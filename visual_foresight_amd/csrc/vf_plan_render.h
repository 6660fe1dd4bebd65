// vf_plan_render.h - plan visualisation: the best plans of a CEM iteration rendered as bytes on the device
// (reference visual_mpc/policy/cem_controllers/pixel_cost_controller.py:107-126: predicted frames as uint8, every
// designated-pixel distribution through a 256-entry colour table), so that only the rendered movies leave it.
//   render_frames    one thread per 16-byte load: (uint8) trunc(frame * 255), four bytes in one 32-bit store
//   render_distrib   one workgroup per (plan, view, step) image, all ndesig channels: plane maximum, then colours
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vf_small_kernels.h"

namespace vf {

constexpr int kRenderThreads = 256;

// the rolled sequence plan k shows; an entry outside the last rollout is clamped, never followed out of bounds
__device__ __forceinline__ long long render_sequence(const int *seq, int k, int last_B) {
    return (long long)min(max(seq[k], 0), last_B - 1);
}

__device__ __forceinline__ uint32_t frame_byte(float v) {
    return (uint32_t)(int)__fmul_rn(v, 255.0f) & 0xffu;       // frames are in [0, 1]: the truncation is the byte
}

// dst [K][ncam][T][H*W*3] bytes <- frames [ncam][Bcap][T][H*W*3] (view_stride floats per view).  blockIdx.y = k * ncam
// + view: the gather by seq[k] is uniform per workgroup; n4 = T * H * W * 3 / 4 loads per (plan, view).
VF_GLOBAL VF_LAUNCH_BOUNDS(kRenderThreads) void
render_frames_kernel(const float *frames, long long view_stride, const int *seq, int last_B, int ncam, int n4,
                     uint32_t *dst) {
    const int i = blockIdx.x * kRenderThreads + threadIdx.x;
    if (i >= n4) return;
    const int k = blockIdx.y / ncam, v = blockIdx.y % ncam;
    const long long b = render_sequence(seq, k, last_B);
    const float4 f = reinterpret_cast<const float4 *>(frames + (long long)v * view_stride + b * 4LL * n4)[i];
    dst[(long long)blockIdx.y * n4 + i] =
        frame_byte(f.x) | (frame_byte(f.y) << 8) | (frame_byte(f.z) << 16) | (frame_byte(f.w) << 24);
}

// dst [K][ncam][ND][T][H*W][3] bytes <- distrib [ncam][Bcap][T][H*W][ND] (un-normalised, channels interleaved).
// One workgroup per (k, view, t).  A thread owns four consecutive pixels of every channel: ND 16-byte loads in,
// three dwords (12 bytes) per channel out.  Per channel d, with p the normalised value vf_export gives
// (distrib_normalised, vf_small_kernels.h):
//     mx = max over the plane of p;  q = p / (mx + 1e-6f)  (float32 add, IEEE float32 division);
//     index = min((int)(q * 256.0f), 255);  pixel = lut[index]
// Pass 1 takes the maxima (lanes by the xor butterfly, the four waves through LDS; a maximum does not depend on the
// order), pass 2 reads the image again and colours it.  The colour table sits in LDS.
template <int ND>
VF_GLOBAL VF_LAUNCH_BOUNDS(kRenderThreads) void
render_distrib_kernel(const float *distrib, long long view_stride, const double *sums, long long step_stride,
                      long long sums_view_stride, int ntiles, const int *seq, int last_B, int ncam, int T, int HW,
                      const uint8_t *lut, uint32_t *dst) {
    __shared__ uint8_t s_lut[256 * 3];
    __shared__ double s_s0[ND];
    __shared__ float s_max[kRenderThreads / 64][ND];
    const int tid = threadIdx.x;
    const int t = blockIdx.x % T, v = (blockIdx.x / T) % ncam, k = blockIdx.x / (T * ncam);
    const long long b = render_sequence(seq, k, last_B);
    for (int i = tid; i < 256 * 3; i += kRenderThreads) s_lut[i] = lut[i];
    if (tid < ND)
        s_s0[tid] = distrib_s0(sums + (long long)t * step_stride + (long long)v * sums_view_stride +
                               (b * ND + tid) * ntiles * 2, ntiles);
    __syncthreads();
    double s0[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) s0[d] = s_s0[d];
    const float4 *src = reinterpret_cast<const float4 *>(distrib + (long long)v * view_stride +
                                                         (b * T + t) * (long long)HW * ND);
    const int groups = HW / 4;      // (H, W multiples of 8)
    float mx[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) mx[d] = 0.0f;      // distributions are non-negative
    for (int g = tid; g < groups; g += kRenderThreads) {
        float val[4 * ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const float4 f = src[g * ND + j];
            val[4 * j] = f.x; val[4 * j + 1] = f.y; val[4 * j + 2] = f.z; val[4 * j + 3] = f.w;
        }
#pragma unroll
        for (int e = 0; e < 4 * ND; ++e) mx[e % ND] = fmaxf(mx[e % ND], distrib_normalised(val[e], s0[e % ND]));
    }
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        for (int off = 32; off > 0; off >>= 1) mx[d] = fmaxf(mx[d], __shfl_xor(mx[d], off, 64));
        if ((tid & 63) == 0) s_max[tid >> 6][d] = mx[d];
    }
    __syncthreads();
    float denom[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) {
        float m = s_max[0][d];
        for (int w = 1; w < kRenderThreads / 64; ++w) m = fmaxf(m, s_max[w][d]);
        denom[d] = __fadd_rn(m, 1e-6f);
    }
    const long long plane_dwords = (long long)HW * 3 / 4;
    uint32_t *out = dst + (((long long)(k * ncam + v) * ND) * T + t) * plane_dwords;    // channel 0; +T planes per channel
    for (int g = tid; g < groups; g += kRenderThreads) {
        float val[4 * ND];
#pragma unroll
        for (int j = 0; j < ND; ++j) {
            const float4 f = src[g * ND + j];
            val[4 * j] = f.x; val[4 * j + 1] = f.y; val[4 * j + 2] = f.z; val[4 * j + 3] = f.w;
        }
#pragma unroll
        for (int d = 0; d < ND; ++d) {
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const float q = __fdiv_rn(distrib_normalised(val[px * ND + d], s0[d]), denom[d]);
                const int idx = min(max((int)__fmul_rn(q, 256.0f), 0), 255);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int byte = px * 3 + c;
                    w[byte >> 2] |= (uint32_t)s_lut[idx * 3 + c] << (8 * (byte & 3));
                }
            }
            uint32_t *o = out + (long long)d * T * plane_dwords + 3LL * g;
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        }
    }
}

}  // namespace vf
