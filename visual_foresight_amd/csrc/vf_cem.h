// vf_cem.h - one CEM iteration on the device: elite selection + Gaussian refit, and sampling of the next candidates.
//
// Specification: visual_foresight_amd/policy/cem_controllers/samplers/philox_gaussian_sampler.py (a float64 NumPy class that
// is a sampler in its own right).  These kernels compute its numbers: elite indices, trial counts, mean and A bit for bit;
// the actions up to the device's float64 log / sin / cos (the only steps that are not correctly rounded on both sides).
//
// Workspace (caller-owned, vf_cem_workspace_bytes; all of it written by cem_refit_kernel or uploaded by the host):
//   int32  R, pad[3]           columns of A in use (D initially, K after a refit)
//   double mean[D]
//   double A[Rmax][D]          A[d, r] at [r][d] (a wave reads one r of all its d at a time), Rmax = max(D, K)
//
//   cem_refit_kernel    ONE workgroup.  The scores [M <= 4096] are staged in LDS; element i's rank is the number of elements
//                       before it in the order (score, index) ascending, NaN last - ranks are distinct, so rank < K names the
//                       elites and their places without a sort.  Then one thread per d: the elites' sum in rank order, the
//                       mean, the column entries (e - mean) / sqrt(K - 1), all float64, each operation rounded once.
//   cem_sample_kernel   one wavefront per sample, four per workgroup, no LDS, no barrier.  Lane l makes Philox block l of the
//                       trial (normals 4l .. 4l+3; R <= 256 = 64 blocks) and owns d = l and d = l + 64 (D <= 128).  The chain
//                       x_d = fma(A[d, r], z_r, x_d) runs r ascending with z_r broadcast from its lane.  The accept vote is
//                       wave-wide; the trial loop is bounded by max_trials and is the only data-dependent loop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vf_conv_mfma.h"

namespace vf {

constexpr int kCemMaxD = 128;           // nactions * adim
constexpr int kCemMaxK = 256;           // elites
constexpr int kCemMaxWidth = 8;         // adim + appended constants
constexpr int kCemMaxM = 4096;          // candidates (the LDS stage of the selection)
constexpr int kCemThreads = 256;
constexpr int kCemWaves = kCemThreads / 64;
constexpr int kCemHeaderBytes = 16;

struct CemParams {
    int nactions, repeat, adim, tail;   // D = nactions * adim, T = nactions * repeat, a row of d_actions has adim + tail floats
    int K, M;
    int max_trials, rejection, zero_first, discrete_mask;
    unsigned seed_lo, seed_hi, call;
    double rej_lim[kCemMaxWidth];       // per action column; +inf = none
    double trunc_lim[kCemMaxWidth];
    double tail_value[kCemMaxWidth];
    const double *scores;               // refit
    const float *actions_in;            // refit
    float *actions_out;                 // sample
    int *elite_index;
    double *elite_score;
    float *elite_plans;
    int *trials, *capped;
    void *workspace;
};

__host__ __device__ inline int cem_rmax(int D, int K) { return D > K ? D : K; }
__host__ __device__ inline size_t cem_workspace_bytes(int D, int K) {
    return (size_t)kCemHeaderBytes + sizeof(double) * (size_t)D * (size_t)(1 + cem_rmax(D, K));
}

// (a, i) before (b, j): scores ascending, NaN after every number, equal scores (and NaNs among themselves) by index
__device__ __forceinline__ bool cem_before(double a, int i, double b, int j) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an == bn ? i < j : bn;
    return a < b || (a == b && i < j);
}

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_refit_kernel(const CemParams p) {
    __shared__ double s_score[kCemMaxM];
    __shared__ int s_elite[kCemMaxK];
    const int tid = threadIdx.x;
    const int D = p.nactions * p.adim, T = p.nactions * p.repeat, W = p.adim + p.tail, K = p.K, M = p.M;
    for (int i = tid; i < M; i += kCemThreads) s_score[i] = p.scores[i];
    __syncthreads();
    for (int i = tid; i < M; i += kCemThreads) {
        const double mine = s_score[i];
        int rank = 0;
        for (int j = 0; j < M; ++j) rank += cem_before(s_score[j], j, mine, i) ? 1 : 0;
        if (rank < K) {
            s_elite[rank] = i;
            p.elite_index[rank] = i;
            p.elite_score[rank] = mine;
        }
    }
    __syncthreads();
    char *ws = static_cast<char *>(p.workspace);
    double *mean = reinterpret_cast<double *>(ws + kCemHeaderBytes);
    double *A = mean + D;
    if (tid == 0) {
        int *head = reinterpret_cast<int *>(ws);
        head[0] = K; head[1] = 0; head[2] = 0; head[3] = 0;
    }
    if (tid < D) {
        const int a = tid / p.adim, c = tid % p.adim;
        const long long at = (long long)(a * p.repeat + p.repeat - 1) * W + c;      // the last step of the held action
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum = __dadd_rn(sum, (double)p.actions_in[(long long)s_elite[k] * T * W + at]);
        const double m = __ddiv_rn(sum, (double)K);
        const double scale = __dsqrt_rn((double)(K - 1));
        mean[tid] = m;
        for (int k = 0; k < K; ++k) {
            const double e = (double)p.actions_in[(long long)s_elite[k] * T * W + at];
            A[(long long)k * D + tid] = __ddiv_rn(__dsub_rn(e, m), scale);
        }
    }
    const int plan = T * W;
    for (int e = tid; e < K * plan; e += kCemThreads) {
        const int k = e / plan;
        p.elite_plans[e] = p.actions_in[(long long)s_elite[k] * plan + (e - k * plan)];
    }
}

__device__ __forceinline__ void cem_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                           unsigned out[4]) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Box-Muller of one word pair: (rho * cos(phi), rho * sin(phi)); every operation rounded on its own
__device__ __forceinline__ void cem_pair(unsigned x, unsigned y, double &zc, double &zs) {
    const double u1 = __ddiv_rn(__dadd_rn((double)x, 1.0), 4294967296.0);
    const double u2 = __ddiv_rn((double)y, 4294967296.0);
    const double rho = __dsqrt_rn(__dmul_rn(-2.0, log(u1)));
    const double phi = __dmul_rn(6.283185307179586, u2);
    zc = __dmul_rn(rho, cos(phi));
    zs = __dmul_rn(rho, sin(phi));
}

__device__ __forceinline__ double cem_clip(double v, double lo, double hi) {     // NaN stays NaN
    return v < lo ? lo : (v > hi ? hi : v);
}

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_sample_kernel(const CemParams p) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kCemWaves + (threadIdx.x >> 6);
    if (i >= p.M) return;               // whole waves leave: nothing below waits for another wave
    const int D = p.nactions * p.adim, T = p.nactions * p.repeat, W = p.adim + p.tail;
    const char *ws = static_cast<const char *>(p.workspace);
    const double *mean = reinterpret_cast<const double *>(ws + kCemHeaderBytes);
    const double *A = mean + D;
    int R = *reinterpret_cast<const int *>(ws);
    R = max(0, min(R, cem_rmax(D, p.K)));       // never past the workspace, whatever the header holds
    const int n_blocks = (R + 3) >> 2;          // <= 64: one per lane
    const int d0 = lane, d1 = lane + 64;
    const bool live0 = d0 < D, live1 = d1 < D;
    const int c0 = live0 ? d0 % p.adim : 0, c1 = live1 ? d1 % p.adim : 0;
    const double m0 = live0 ? mean[d0] : 0.0, m1 = live1 ? mean[d1] : 0.0;
    const double lim0 = p.rej_lim[c0], lim1 = p.rej_lim[c1];
    double x0 = m0, x1 = m1;
    int n = 0;
    bool accepted = false;
    for (; n < p.max_trials; ++n) {
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        if (lane < n_blocks) {
            unsigned w[4];
            cem_philox((unsigned)lane, (unsigned)n, (unsigned)i, p.call, p.seed_lo, p.seed_hi, w);
            cem_pair(w[0], w[1], z[0], z[1]);
            cem_pair(w[2], w[3], z[2], z[3]);
        }
        x0 = m0; x1 = m1;
        for (int j = 0; j < n_blocks; ++j) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = 4 * j + q;
                const double zr = __shfl(z[q], j);
                if (r < R) {
                    const double a0 = live0 ? A[(long long)r * D + d0] : 0.0;
                    const double a1 = live1 ? A[(long long)r * D + d1] : 0.0;
                    x0 = fma(a0, zr, x0);
                    x1 = fma(a1, zr, x1);
                }
            }
        }
        const bool ok = (!live0 || fabs(x0) <= lim0) && (!live1 || fabs(x1) <= lim1);
        if (!p.rejection || __all(ok)) { accepted = true; break; }
    }
    if (lane == 0) {
        p.trials[i] = accepted ? n + 1 : p.max_trials;
        p.capped[i] = accepted ? 0 : 1;
    }
    float *out = p.actions_out + (long long)i * T * W;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int d = half ? d1 : d0, c = half ? c1 : c0;
        if (d >= D) continue;
        double v = half ? x1 : x0;
        const double lim = half ? lim1 : lim0;
        if (!accepted) v = cem_clip(v, -lim, lim);
        if ((p.discrete_mask >> c) & 1) v = cem_clip(floor(v), 0.0, 4.0);
        const double tl = p.trunc_lim[c];
        v = cem_clip(v, -tl, tl);
        if (p.zero_first && i == 0) v = 0.0;
        const float f = (float)v;
        const int a = d / p.adim;
        for (int q = 0; q < p.repeat; ++q) out[(a * p.repeat + q) * W + c] = f;
    }
    for (int e = lane; e < T * p.tail; e += 64) {
        const int t = e / p.tail, k = e % p.tail;
        out[t * W + p.adim + k] = (float)p.tail_value[k];
    }
}

}  // namespace vf
