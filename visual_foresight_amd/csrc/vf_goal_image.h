// vf_goal_image.h - goal-image cost: mean squared error between predicted frames and a goal picture
// (reference visual_mpc/policy/cem_controllers/goal_im_controller.py:93), reduced on the device.
//   goal_mse         one workgroup per (sequence, view, step) image: streams the resident frame and the goal,
//                    writes mse[b][view][t] (float64)
//   goal_scores      one thread per action: time weighting, mean over latent draws, mean over views
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vf_conv_mfma.h"

namespace vf {

constexpr int kGoalThreads = 256;

// mse[(b * ncam + v) * T + t] = sum over the image's n4 * 4 values of (frame - goal)^2 / (n4 * 4),  t = t0 + step.
// frames: the engine's resident predictions [ncam][Bcap][T][H*W*3] (view_stride floats per view); goal [ncam][H*W*3].
// Difference and square are float64 (both operands are float32, so every term is the exact square of the exact
// difference rounded once); terms are added per lane in the order the lane meets them (16-byte load i = lane,
// lane + 256, ..., components x, y, z, w), the 64 lanes of a wave by the xor butterfly, the four waves through LDS
// in wave order.  The tree depends on n4 = H * W * 3 / 4 alone - not on the batch, the chunk or the device lane - so
// a sequence's cost has the same bits wherever and with whatever neighbours it is rolled.  A last partial sweep of
// the 256 threads is predicated (no load, nothing added), not a second code path.
VF_GLOBAL VF_LAUNCH_BOUNDS(kGoalThreads) void
goal_mse_kernel(const float *frames, long long view_stride, const float *goal, int ncam, int T, int n4, int t0,
                int n_steps, double *mse) {
    __shared__ double wave_part[kGoalThreads / 64];
    const int tid = threadIdx.x;
    const int step = blockIdx.x % n_steps;
    const int v = (blockIdx.x / n_steps) % ncam;
    const long long b = blockIdx.x / (n_steps * ncam);
    const int t = t0 + step;
    const float4 *f4 = reinterpret_cast<const float4 *>(frames + (long long)v * view_stride + (b * T + t) * 4LL * n4);
    const float4 *g4 = reinterpret_cast<const float4 *>(goal + (long long)v * 4LL * n4);
    double acc = 0.0;
    for (int i = tid; i < n4; i += kGoalThreads) {
        const float4 f = f4[i], g = g4[i];
        const double dx = (double)f.x - (double)g.x, dy = (double)f.y - (double)g.y;
        const double dz = (double)f.z - (double)g.z, dw = (double)f.w - (double)g.w;
        acc += dx * dx;
        acc += dy * dy;
        acc += dz * dz;
        acc += dw * dw;
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) wave_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = wave_part[0];
        for (int w = 1; w < kGoalThreads / 64; ++w) s += wave_part[w];
        mse[(b * ncam + v) * T + t] = s / (4.0 * (double)n4);
    }
}

// Per action a (n_draws consecutive rolled sequences) and view v:
//   steps_mode 0: e = mse[T-1];   steps_mode 1: e = sum_t w_t mse[t] / sum_t w_t,  w = (1, ..., 1, finalweight)
// averaged over the draws in draw order; score = e of view 0 (first_view_only) or the plain mean over views in view
// order.  cost_per_step (optional) [A][ncam][T] = mse averaged over the draws (the caller has had every step reduced).
// A non-zero *status poisons every output with NaN, as scores_kernel does.
VF_GLOBAL void goal_scores_kernel(const double *mse, int n_actions, int n_draws, int ncam, int T, int steps_mode,
                                   float finalweight, int first_view_only, const int *status, double *scores,
                                   double *scores_per_view, double *cost_per_step) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n_actions) return;
    const bool poisoned = status && *status != 0;
    const double nan = __builtin_nan("");
    double total = 0.0, first = 0.0;
    for (int v = 0; v < ncam; ++v) {
        double over_draws = 0.0;
        for (int j = 0; j < n_draws; ++j) {
            const double *m = mse + (((long long)a * n_draws + j) * ncam + v) * T;
            if (steps_mode == 0) {
                over_draws += m[T - 1];
            } else {
                double acc = 0.0, wsum = 0.0;
                for (int t = 0; t < T; ++t) {
                    const double w = (t == T - 1) ? (double)finalweight : 1.0;
                    acc += w * m[t];
                    wsum += w;
                }
                over_draws += acc / wsum;
            }
        }
        const double e = over_draws / n_draws;
        if (scores_per_view) scores_per_view[(long long)a * ncam + v] = poisoned ? nan : e;
        if (cost_per_step)
            for (int t = 0; t < T; ++t) {
                double s = 0.0;
                for (int j = 0; j < n_draws; ++j) s += mse[(((long long)a * n_draws + j) * ncam + v) * T + t];
                cost_per_step[((long long)a * ncam + v) * T + t] = poisoned ? nan : s / n_draws;
            }
        if (v == 0) first = e;
        total += e;
    }
    const double out = first_view_only ? first : total / ncam;
    scores[a] = poisoned ? nan : out;
}

}  // namespace vf
