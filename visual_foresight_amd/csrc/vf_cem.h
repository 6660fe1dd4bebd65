// vf_cem.h - one CEM iteration on the device: elite selection + refit, and sampling of the next candidates, for the Gaussian
// proposal (first part), for the time-correlated noise proposal (second part) and for the folding proposal (third part, which
// shares the Gaussian workspace and refit and adds a sampling kernel); the fourth part draws a stochastic predictor's latents
// and folds them into the candidates; the fifth is the autograsp proposal, the Gaussian one with a derived gripper column.
// The later parts' header comments say what differs from the first.  Every piece of arithmetic two kernels share is one
// __device__ __forceinline__ function here (cem_select_elites, cem_fit_factor, cem_copy_elites, cem_normals, cem_gauss,
// cem_chain, cem_store_held, cem_fill_tail, cem_draw, cem_emit, cem_store_moves), as the float64 twins share philox4x32_10,
// standard_normals, fit_factor and draw: these lines are the numerical contract with them, each float64 operation the
// explicit single-rounding intrinsic or fma, in one order (the build keeps -ffp-contract=off).  A function that shuffles or
// votes is called by all 64 lanes of a wave.
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

// The elites of scores [M] by counting (one workgroup, all of it): stages the scores in s_score [M], leaves the index of
// rank k in s_elite[k] and writes elite_index / elite_score [K].  Returns behind a barrier.
__device__ __forceinline__ void cem_select_elites(const double *scores, int M, int K, double *s_score, int *s_elite,
                                                  int *elite_index, double *elite_score) {
    const int tid = threadIdx.x;
    for (int i = tid; i < M; i += kCemThreads) s_score[i] = scores[i];
    __syncthreads();
    for (int i = tid; i < M; i += kCemThreads) {
        const double mine = s_score[i];
        int rank = 0;
        for (int j = 0; j < M; ++j) rank += cem_before(s_score[j], j, mine, i) ? 1 : 0;
        if (rank < K) {
            s_elite[rank] = i;
            elite_index[rank] = i;
            elite_score[rank] = mine;
        }
    }
    __syncthreads();
}

// The factor fit of dimension d (one thread): the elites' value of it lies at `at` of their plans of `plan` floats, `sum` is
// their sum in rank order.  mean[d] = sum / K, A[k][d] = (e_k - mean) / sqrt(K - 1).
__device__ __forceinline__ void cem_fit_factor(const float *actions, const int *s_elite, int K, int plan, long long at, double sum,
                                               int D, int d, double *mean, double *A) {
    const double m = __ddiv_rn(sum, (double)K);
    const double scale = __dsqrt_rn((double)(K - 1));
    mean[d] = m;
    for (int k = 0; k < K; ++k) {
        const double e = (double)actions[(long long)s_elite[k] * plan + at];
        A[(long long)k * D + d] = __ddiv_rn(__dsub_rn(e, m), scale);
    }
}

// elite_plans [K][plan]: the elites' plans in rank order (one workgroup, all of it)
__device__ __forceinline__ void cem_copy_elites(const float *actions, const int *s_elite, int K, int plan, float *elite_plans) {
    for (int e = threadIdx.x; e < K * plan; e += kCemThreads) {
        const int k = e / plan;
        elite_plans[e] = actions[(long long)s_elite[k] * plan + (e - k * plan)];
    }
}

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_refit_kernel(const CemParams p) {
    __shared__ double s_score[kCemMaxM];
    __shared__ int s_elite[kCemMaxK];
    const int tid = threadIdx.x;
    const int D = p.nactions * p.adim, T = p.nactions * p.repeat, W = p.adim + p.tail, K = p.K, M = p.M;
    const int plan = T * W;
    cem_select_elites(p.scores, M, K, s_score, s_elite, p.elite_index, p.elite_score);
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
        for (int k = 0; k < K; ++k) sum = __dadd_rn(sum, (double)p.actions_in[(long long)s_elite[k] * plan + at]);
        cem_fit_factor(p.actions_in, s_elite, K, plan, at, sum, D, tid, mean, A);
    }
    cem_copy_elites(p.actions_in, s_elite, K, plan, p.elite_plans);
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

// Philox block `block` of (trial, sample, call) as four standard normals
__device__ __forceinline__ void cem_normals(unsigned block, unsigned trial, unsigned sample, unsigned call, unsigned seed_lo,
                                            unsigned seed_hi, double z[4]) {
    unsigned w[4];
    cem_philox(block, trial, sample, call, seed_lo, seed_hi, w);
    cem_pair(w[0], w[1], z[0], z[1]);
    cem_pair(w[2], w[3], z[2], z[3]);
}

// The Gaussian workspace as a sampling kernel reads it
struct CemGauss {
    int R, n_blocks;                    // columns of A in use; their Philox blocks (<= 64: one per lane)
    const double *mean, *A;
};
__device__ __forceinline__ CemGauss cem_gauss(const void *workspace, int D, int K) {
    const char *ws = static_cast<const char *>(workspace);
    CemGauss g;
    g.R = max(0, min(*reinterpret_cast<const int *>(ws), cem_rmax(D, K)));      // never past the workspace, whatever the header holds
    g.n_blocks = (g.R + 3) >> 2;
    g.mean = reinterpret_cast<const double *>(ws + kCemHeaderBytes);
    g.A = g.mean + D;
    return g;
}

// The factor-form chain of the lane's two dimensions, d = lane and lane + 64: x_d = fma(A[d, r], z_r, x_d) for r ascending
// from the caller's x_d, z_r being z[r % 4] of lane r / 4 (every lane of the wave calls this: the shuffles are wave-wide).
__device__ __forceinline__ void cem_chain(const CemGauss &g, int D, int lane, const double z[4], double &x0, double &x1) {
    const int d0 = lane, d1 = lane + 64;
    const bool live0 = d0 < D, live1 = d1 < D;
    for (int j = 0; j < g.n_blocks; ++j) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = 4 * j + q;
            const double zr = __shfl(z[q], j);
            if (r < g.R) {
                const double a0 = live0 ? g.A[(long long)r * D + d0] : 0.0;
                const double a1 = live1 ? g.A[(long long)r * D + d1] : 0.0;
                x0 = fma(a0, zr, x0);
                x1 = fma(a1, zr, x1);
            }
        }
    }
}

// column c of the `repeat` steps that hold action a of a sample's rows `out` of W floats
__device__ __forceinline__ void cem_store_held(float *out, int a, int repeat, int W, int c, float f) {
    for (int q = 0; q < repeat; ++q) out[(a * repeat + q) * W + c] = f;
}

// the appended constants: columns col .. col + count - 1 of all T rows of a sample take value[0 .. count - 1] (the wave's lanes)
__device__ __forceinline__ void cem_fill_tail(float *out, int lane, int T, int W, int col, int count, const double *value) {
    for (int e = lane; e < T * count; e += 64) {
        const int t = e / count, k = e % count;
        out[t * W + col + k] = (float)value[k];
    }
}

__device__ __forceinline__ double cem_clip(double v, double lo, double hi) {     // NaN stays NaN
    return v < lo ? lo : (v > hi ? hi : v);
}

// What a lane holds of its sample after the trials: its two dimensions, their action columns and rejection limits, the
// values of the accepted (or last) trial, the trials taken.  cem_sample_kernel and cem_sample_autograsp_kernel share it.
struct CemLane {
    int d0, d1, c0, c1;
    double x0, x1, lim0, lim1;
    int n;
    bool accepted;
};

// The trials of sample i (every lane of its wave calls this: the shuffles and the vote are wave-wide).
__device__ __forceinline__ CemLane cem_draw(const CemParams &p, int lane, int i) {
    const int D = p.nactions * p.adim;
    const CemGauss g = cem_gauss(p.workspace, D, p.K);
    CemLane s;
    s.d0 = lane; s.d1 = lane + 64;
    const int d0 = s.d0, d1 = s.d1;
    const bool live0 = d0 < D, live1 = d1 < D;
    s.c0 = live0 ? d0 % p.adim : 0; s.c1 = live1 ? d1 % p.adim : 0;
    const double m0 = live0 ? g.mean[d0] : 0.0, m1 = live1 ? g.mean[d1] : 0.0;
    const double lim0 = p.rej_lim[s.c0], lim1 = p.rej_lim[s.c1];
    double x0 = m0, x1 = m1;
    int n = 0;
    bool accepted = false;
    for (; n < p.max_trials; ++n) {
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        if (lane < g.n_blocks) cem_normals((unsigned)lane, (unsigned)n, (unsigned)i, p.call, p.seed_lo, p.seed_hi, z);
        x0 = m0; x1 = m1;
        cem_chain(g, D, lane, z, x0, x1);
        const bool ok = (!live0 || fabs(x0) <= lim0) && (!live1 || fabs(x1) <= lim1);
        if (!p.rejection || __all(ok)) { accepted = true; break; }
    }
    s.x0 = x0; s.x1 = x1; s.lim0 = lim0; s.lim1 = lim1;
    s.n = n; s.accepted = accepted;
    return s;
}

// The float32 value a lane stores for its dimension of `half`: clipped when capped, discretised, truncated, zeroed
__device__ __forceinline__ float cem_emit(const CemParams &p, const CemLane &s, int half, int i) {
    const int c = half ? s.c1 : s.c0;
    double v = half ? s.x1 : s.x0;
    const double lim = half ? s.lim1 : s.lim0;
    if (!s.accepted) v = cem_clip(v, -lim, lim);
    if ((p.discrete_mask >> c) & 1) v = cem_clip(floor(v), 0.0, 4.0);
    const double tl = p.trunc_lim[c];
    v = cem_clip(v, -tl, tl);
    if (p.zero_first && i == 0) v = 0.0;
    return (float)v;
}

// What cem_draw left goes out: trials / capped of sample i (lane 0) and the lane's two dimensions over their held steps of
// the sample's rows `out`; f[half] is what the lane stored (0 where it owns no dimension).
__device__ __forceinline__ void cem_store_moves(const CemParams &p, const CemLane &s, int lane, int i, float *out, float f[2]) {
    const int D = p.nactions * p.adim, W = p.adim + p.tail;
    if (lane == 0) {
        p.trials[i] = s.accepted ? s.n + 1 : p.max_trials;
        p.capped[i] = s.accepted ? 0 : 1;
    }
    f[0] = f[1] = 0.f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int d = half ? s.d1 : s.d0, c = half ? s.c1 : s.c0;
        if (d >= D) continue;
        f[half] = cem_emit(p, s, half, i);
        cem_store_held(out, d / p.adim, p.repeat, W, c, f[half]);
    }
}

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_sample_kernel(const CemParams p) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kCemWaves + (threadIdx.x >> 6);
    if (i >= p.M) return;               // whole waves leave: nothing below waits for another wave
    const int T = p.nactions * p.repeat, W = p.adim + p.tail;
    const CemLane s = cem_draw(p, lane, i);
    float *out = p.actions_out + (long long)i * T * W;
    float f[2];
    cem_store_moves(p, s, lane, i, out, f);
    cem_fill_tail(out, lane, T, W, p.adim, p.tail, p.tail_value);
}

// ------------------------------------------------------------------ the correlated-noise proposal
// Specification: samplers/philox_correlated_sampler.py.  Elites, the plain mean and A bit for bit; soft and centre up to the
// device's float64 exp, the actions up to its log / sin / cos.
//
// Workspace (caller-owned, cem_corr_workspace_bytes; the host uploads the header, cem_soft_refit_kernel writes the rest):
//   int32  R, centre_valid, pad[2]     R: columns of A in use (K after a refit with refit_cov, else 0)
//   double centre[D]                   the elites' soft mean
//   double mean[D]                     their plain mean (refit_cov only; A is about it)
//   double soft[K]                     their weights
//   double A[K][D]                     refit_cov only: A[d, k] at [k][d]
//
//   cem_soft_refit_kernel   cem_refit_kernel with soft_k staged in LDS and the centre beside the fit (refit_cov only: the fit).
//   cem_sample_corr_kernel  waves and lanes as cem_sample_kernel, one trial of D normals (<= 32 blocks).  The shaped values go
//                           to the wave's LDS strip, lanes c < adim run the serial AR(1) chain of their column in it, every
//                           lane adds the centre.  No data-dependent loop; the only barriers are the wave's own.
struct CemCorrParams {
    int nactions, adim, tail, K, M;
    int refit_cov, has_first_prev;
    unsigned seed_lo, seed_hi, call;
    double kappa, beta_0, beta_1;
    double std[kCemMaxWidth], bias[kCemMaxWidth], first_prev[kCemMaxWidth], tail_value[kCemMaxWidth];
    const double *scores;               // refit
    const float *actions_in;            // refit
    float *actions_out;                 // sample
    int *elite_index;
    double *elite_score;
    float *elite_plans;
    void *workspace;
};

__host__ __device__ inline size_t cem_corr_workspace_bytes(int D, int K, bool refit_cov) {
    return (size_t)kCemHeaderBytes + sizeof(double) * ((size_t)2 * D + (size_t)K + (refit_cov ? (size_t)K * (size_t)D : 0));
}

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_soft_refit_kernel(const CemCorrParams p) {
    __shared__ double s_score[kCemMaxM];
    __shared__ int s_elite[kCemMaxK];
    __shared__ double s_soft[kCemMaxK];
    const int tid = threadIdx.x;
    const int D = p.nactions * p.adim, W = p.adim + p.tail, K = p.K, M = p.M;
    const int plan = p.nactions * W;
    cem_select_elites(p.scores, M, K, s_score, s_elite, p.elite_index, p.elite_score);
    char *ws = static_cast<char *>(p.workspace);
    double *centre = reinterpret_cast<double *>(ws + kCemHeaderBytes);
    double *mean = centre + D;
    double *soft = mean + D;
    double *A = soft + K;
    const double g0 = -s_score[s_elite[0]];
    for (int k = tid; k < K; k += kCemThreads) {
        const double v = exp(__dmul_rn(p.kappa, __dsub_rn(-s_score[s_elite[k]], g0)));
        s_soft[k] = v;
        soft[k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        int *head = reinterpret_cast<int *>(ws);
        head[0] = p.refit_cov ? K : 0; head[1] = 1; head[2] = 0; head[3] = 0;
    }
    if (tid < D) {
        const long long at = (long long)(tid / p.adim) * W + tid % p.adim;
        double num = 0.0, den = 0.0, sum = 0.0;
        for (int k = 0; k < K; ++k) {
            const double e = (double)p.actions_in[(long long)s_elite[k] * plan + at];
            num = __dadd_rn(num, __dmul_rn(e, s_soft[k]));
            den = __dadd_rn(den, s_soft[k]);
            sum = __dadd_rn(sum, e);
        }
        centre[tid] = __ddiv_rn(num, __dadd_rn(den, 1e-4));
        if (p.refit_cov) cem_fit_factor(p.actions_in, s_elite, K, plan, at, sum, D, tid, mean, A);
    }
    cem_copy_elites(p.actions_in, s_elite, K, plan, p.elite_plans);
}

// what the other lanes of the wave wrote to LDS is visible behind this
__device__ __forceinline__ void cem_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_sample_corr_kernel(const CemCorrParams p) {
    __shared__ double s_strip[kCemWaves][kCemMaxD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * kCemWaves + wave;
    if (i >= p.M) return;               // whole waves leave: nothing below waits for another wave
    const int D = p.nactions * p.adim, W = p.adim + p.tail, K = p.K;
    const char *ws = static_cast<const char *>(p.workspace);
    const int *head = reinterpret_cast<const int *>(ws);
    const double *centre = reinterpret_cast<const double *>(ws + kCemHeaderBytes);
    const double *A = centre + 2 * D + K;
    const int R = p.refit_cov ? max(0, min(head[0], K)) : 0;     // never past the workspace, whatever the header holds
    const bool centred = head[1] != 0;
    const int n_blocks = (D + 3) >> 2;          // <= 32: one per lane
    const int d0 = lane, d1 = lane + 64;
    const bool live0 = d0 < D, live1 = d1 < D;
    const int c0 = live0 ? d0 % p.adim : 0, c1 = live1 ? d1 % p.adim : 0;
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < n_blocks) cem_normals((unsigned)lane, 0u, (unsigned)i, p.call, p.seed_lo, p.seed_hi, z);
    double s0 = 0.0, s1 = 0.0;
    if (R == 0) {
        double w0 = 0.0, w1 = 0.0;      // w_d lies in lane d / 4 as z[d % 4]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double v0 = __shfl(z[q], (d0 >> 2) & 63), v1 = __shfl(z[q], (d1 >> 2) & 63);
            if ((d0 & 3) == q) w0 = v0;
            if ((d1 & 3) == q) w1 = v1;
        }
        s0 = __dadd_rn(__dmul_rn(w0, p.std[c0]), p.bias[c0]);
        s1 = __dadd_rn(__dmul_rn(w1, p.std[c1]), p.bias[c1]);
    } else {
        double y[4] = {0.0, 0.0, 0.0, 0.0};     // y_k of k = lane + 64 j (K <= 256)
        for (int b = 0; b < n_blocks; ++b) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d = 4 * b + q;
                const double wd = __shfl(z[q], b);
                if (d < D) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = lane + 64 * j;
                        if (k < R) y[j] = fma(wd, A[(long long)k * D + d], y[j]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (int l = 0; l < 64; ++l) {
                const int k = 64 * j + l;
                if (k >= R) break;              // (uniform)
                const double yk = __shfl(y[j], l);
                if (live0) s0 = fma(A[(long long)k * D + d0], yk, s0);
                if (live1) s1 = fma(A[(long long)k * D + d1], yk, s1);
            }
        }
    }
    double *strip = s_strip[wave];
    if (live0) strip[d0] = s0;
    if (live1) strip[d1] = s1;
    cem_wave_sync();
    if (lane < p.adim) {                // the serial chain of column `lane`, in place: step a reads s_a before it writes o_a
        double prev = p.has_first_prev ? p.first_prev[lane] : strip[(p.nactions - 1) * p.adim + lane];
        for (int a = 0; a < p.nactions; ++a) {
            const double o = __dadd_rn(__dmul_rn(p.beta_0, strip[a * p.adim + lane]), __dmul_rn(p.beta_1, prev));
            strip[a * p.adim + lane] = o;
            prev = o;
        }
    }
    cem_wave_sync();
    float *out = p.actions_out + (long long)i * p.nactions * W;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int d = half ? d1 : d0, c = half ? c1 : c0;
        if (d >= D) continue;
        double v = strip[d];
        if (centred) v = __dadd_rn(v, centre[d]);
        out[(d / p.adim) * W + c] = (float)v;
    }
    cem_fill_tail(out, lane, p.nactions, W, p.adim, p.tail, p.tail_value);
}

// ------------------------------------------------------------------ the folding proposal
// Specification: samplers/philox_folding_sampler.py.  The proposal, its workspace and its refit are the Gaussian one's
// (cem_refit_kernel with adim = 4); only the sampling differs.  The actions up to the device's log / sin / cos.
//
//   cem_sample_fold_kernel  waves and lanes as cem_sample_kernel (both dimensions of a lane are of channel c = l & 3), no
//                           data-dependent loop.  Sample i < n_scripted is TWO_PLACES, i < 2 n_scripted ONE_PLACE, the rest
//                           plain (a wave-uniform branch).  Plain: trial 0 through cem_chain.  Scripted: the places from trial 1,
//                           block 0 (every lane makes it); then per scripted step s (trial 2 + s) the chain
//                           y_c = sum_r A[c, r] z_r from 0.0 over row c of A, v_c = m_c + g_c y_c, and a lane keeps the value
//                           of the step its action index maps to (ONE_PLACE holds its last step, TWO_PLACES leaves zero).
constexpr int kCemFoldAdim = 4;
constexpr int kCemFoldSteps = 5;        // the longer script (TWO_PLACES); ONE_PLACE has 4

struct CemFoldParams {
    int nactions, repeat, tail, K, M, n_scripted;
    unsigned seed_lo, seed_hi, call;
    double start_xy[2], max_shift[3], tail_value[kCemMaxWidth];
    float *actions_out;
    const void *workspace;
};

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_sample_fold_kernel(const CemFoldParams p) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kCemWaves + (threadIdx.x >> 6);
    if (i >= p.M) return;               // whole waves leave: nothing below waits for another wave
    const int D = p.nactions * kCemFoldAdim, T = p.nactions * p.repeat, W = kCemFoldAdim + p.tail;
    const CemGauss g = cem_gauss(p.workspace, D, p.K);
    const int d0 = lane, d1 = lane + 64;
    const int c = lane & 3, a0 = lane >> 2, a1 = a0 + 16;
    double x0 = 0.0, x1 = 0.0;
    if (i >= 2 * p.n_scripted) {                // plain: the Gaussian sampler's unrejected draw
        double z[4] = {0.0, 0.0, 0.0, 0.0};
        if (lane < g.n_blocks) cem_normals((unsigned)lane, 0u, (unsigned)i, p.call, p.seed_lo, p.seed_hi, z);
        x0 = d0 < D ? g.mean[d0] : 0.0;
        x1 = d1 < D ? g.mean[d1] : 0.0;
        cem_chain(g, D, lane, z, x0, x1);
    } else {
        const bool two = i < p.n_scripted;
        unsigned pw[4];
        cem_philox(0u, 1u, (unsigned)i, p.call, p.seed_lo, p.seed_hi, pw);
        // the carries of this lane's channel (x or y; lift and rotation have none): start -> first place -> second place
        const double start = p.start_xy[c & 1];
        const double first = __ddiv_rn((double)pw[c & 1], 4294967296.0);
        const double second = __ddiv_rn((double)pw[2 + (c & 1)], 4294967296.0);
        const double rep = (double)p.repeat;
        const double way0 = __ddiv_rn(__dsub_rn(first, start), rep);
        const double way1 = __ddiv_rn(__dsub_rn(second, first), rep);
        const int n_steps = two ? kCemFoldSteps : kCemFoldSteps - 1;
        // the scripted step an action index takes: TWO_PLACES none past its script (-1), ONE_PLACE its last
        const int s0 = a0 < n_steps ? a0 : (two ? -1 : n_steps - 1);
        const int s1 = two ? -1 : n_steps - 1;  // (a1 >= 16 is past either script)
        for (int s = 0; s < n_steps; ++s) {
            double z[4] = {0.0, 0.0, 0.0, 0.0};
            if (lane < g.n_blocks) cem_normals((unsigned)lane, (unsigned)(2 + s), (unsigned)i, p.call, p.seed_lo, p.seed_hi, z);
            // the one-row chain stays written out: through cem_chain it would carry a second, dead fma per step (d = c + 64)
            double y = 0.0;
            for (int j = 0; j < g.n_blocks; ++j) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int r = 4 * j + q;
                    const double zr = __shfl(z[q], j);
                    if (r < g.R) y = fma(g.A[(long long)r * D + c], zr, y);
                }
            }
            const bool carry = two ? (s == 0 || s == 3) : s == 1;
            const double lift = two ? ((s == 1 || s == 4) ? -1.0 : 1.0) : (s < 2 ? 1.0 : (s == 2 ? -1.0 : 0.0));
            const double way = (two && s == 3) ? way1 : way0;
            const double m = c < 2 ? (carry ? way : 0.0) : (c == 2 ? lift : 0.0);
            const double g = (carry || c == 2) ? 1.0 : (c < 2 ? 0.31622776601683794 : 0.7071067811865476);   // sqrt(.1), sqrt(.5)
            const double v = __dadd_rn(m, __dmul_rn(g, y));
            if (s == s0) x0 = v;
            if (s == s1) x1 = v;
        }
    }
    float *out = p.actions_out + (long long)i * T * W;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int d = half ? d1 : d0;
        if (d >= D) continue;
        double v = half ? x1 : x0;
        if (c < 3) v = cem_clip(v, -p.max_shift[c], p.max_shift[c]);
        cem_store_held(out, half ? a1 : a0, p.repeat, W, c, (float)v);
    }
    cem_fill_tail(out, lane, T, W, kCemFoldAdim, p.tail, p.tail_value);
}

// ------------------------------------------------------------------ latent draws of the stochastic predictor
// Specification: video_prediction/stochastic_predictor.py, philox_latents / fold_latents.  The latents up to the device's
// log / sin / cos; the fold is copying.
//
//   cem_latents_kernel       one wavefront per draw d.  The N = T * zdim normals of draw d are those of the counter
//                            {block, 0xFFFFFFFF, d, call}: a trial word no sampler uses, so that equal seeds and call
//                            numbers share no counter with the candidates.  Lane l makes blocks
//                            l, l + 64, ... < n_blocks (host-known: no data-dependent loop) and stores its four normals,
//                            each float64 rounded once to float32.
//   cem_fold_latents_kernel  row a * n_latent + d of the engine's sequences is [actions[a] | z[d]] per step: one output
//                            element per thread in a grid-stride loop (a float4 when width and zdim are multiples of four,
//                            where every piece of a row is 16-byte aligned; else a float).
constexpr unsigned kCemLatentTrial = 0xFFFFFFFFu;
constexpr int kCemFoldMaxBlocks = 1 << 16;     // the grid of the fold: the loop strides over the rest

struct CemLatentParams {
    int n_latent, n_blocks;
    long long N;                        // T * zdim
    unsigned seed_lo, seed_hi, call;
    float *z;
};

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_latents_kernel(const CemLatentParams p) {
    const int lane = threadIdx.x & 63;
    const int d = blockIdx.x * kCemWaves + (threadIdx.x >> 6);
    if (d >= p.n_latent) return;
    float *out = p.z + (long long)d * p.N;
    for (int b = lane; b < p.n_blocks; b += 64) {
        double z[4];
        cem_normals((unsigned)b, kCemLatentTrial, (unsigned)d, p.call, p.seed_lo, p.seed_hi, z);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long e = 4LL * b + q;
            if (e < p.N) out[e] = (float)z[q];
        }
    }
}

struct CemFoldLatentParams {
    int n_latent, T, width, zdim;
    long long total;                    // output elements: floats, or float4s with VEC
    const float *actions, *z;
    float *seqs;
};

template <bool VEC>
VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_fold_latents_kernel(const CemFoldLatentParams p) {
    constexpr int kPer = VEC ? 4 : 1;
    const int W = p.width / kPer, Z = p.zdim / kPer, RW = W + Z;
    const long long stride = (long long)gridDim.x * kCemThreads;
    for (long long g = (long long)blockIdx.x * kCemThreads + threadIdx.x; g < p.total; g += stride) {
        const long long step = g / RW;                  // (row, t) of the output
        const int q = (int)(g - step * RW);
        const long long row = step / p.T;
        const int t = (int)(step - row * p.T);
        const long long a = row / p.n_latent;
        const int d = (int)(row - a * p.n_latent);
        const long long src = q < W ? (a * p.T + t) * W + q : ((long long)d * p.T + t) * Z + (q - W);
        const float *from = q < W ? p.actions : p.z;
        if (VEC) reinterpret_cast<float4 *>(p.seqs)[g] = reinterpret_cast<const float4 *>(from)[src];
        else p.seqs[g] = from[src];
    }
}

// ------------------------------------------------------------------ the autograsp proposal
// Specification: samplers/philox_autograsp_sampler.py.  The moves (columns 0 .. adim - 1), their workspace and their refit are
// the Gaussian proposal's: cem_draw / cem_emit above and cem_refit_kernel, under a CemParams whose adim counts the moves and
// whose tail counts the gripper column (column adim) and the appended constants behind it.  The gripper column is derived
// from the float32 moves the kernel stores, so it equals the specification's on those moves bit for bit whatever the
// device's log / sin / cos did to them.
//
//   cem_grip_share_kernel        ONE workgroup, share mode only: share[t] = float32(count_t) / float32(K), count_t the
//                                elites whose gripper value at step t is the close command - one thread per step in a loop,
//                                so that the sampling kernel reads T floats, not K * T elite values per sample.
//   cem_sample_autograsp_kernel  the moves as cem_sample_kernel (its trial loop stays the only data-dependent loop).  Steps
//                                go in rounds of 64, lane l owning step 64 * round + l.  Height mode: EVERY lane
//                                runs the serial chain c_t = c_(t-1) + float64(z_t) * norm, h_t = c_t + state_z (z_t fetched
//                                by __shfl from the lane that owns the lift of step t's action, every operation rounded
//                                once, the latch carried along) and keeps the decision of its own step - a shuffle scan
//                                would round differently.  The uniform of step t is word t % 4 of Philox block t / 4 under
//                                trial 0xFFFFFFFE (no sampler's trial, not the latents' 0xFFFFFFFF): it flips the step with
//                                deviation_prob (none drawn when that is 0) or, in share mode, shuts it when u < share[t].
constexpr unsigned kCemGripTrial = 0xFFFFFFFEu;
constexpr int kCemGripHeight = 0, kCemGripShare = 1;
constexpr int kCemGripLift = 2;         // the move channel the height follows

struct CemGripParams {
    int mode, reopen;
    double state_z, norm, z_thresh, deviation_prob;
    float close_cmd, open_cmd;
    const float *elite_plans;           // share mode: [K][T][W]
    float *share;                       // share mode: [T]
};

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_grip_share_kernel(const CemGripParams g, int K, int T, int W, int col) {
    for (int t = threadIdx.x; t < T; t += kCemThreads) {
        int count = 0;
        for (int k = 0; k < K; ++k) count += g.elite_plans[((long long)k * T + t) * W + col] == g.close_cmd ? 1 : 0;
        g.share[t] = __fdiv_rn((float)count, (float)K);
    }
}

VF_GLOBAL VF_LAUNCH_BOUNDS(kCemThreads) void cem_sample_autograsp_kernel(const CemParams p, const CemGripParams g) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kCemWaves + (threadIdx.x >> 6);
    if (i >= p.M) return;               // whole waves leave: nothing below waits for another wave
    const int T = p.nactions * p.repeat, W = p.adim + p.tail;
    const CemLane s = cem_draw(p, lane, i);
    float *out = p.actions_out + (long long)i * T * W;
    float f[2];                         // what this lane stores for d0 and d1
    cem_store_moves(p, s, lane, i, out, f);
    const bool by_height = g.mode == kCemGripHeight;
    const bool draws = !by_height || g.deviation_prob > 0.0;
    double c = 0.0;
    bool latched = false;
    for (int base = 0; base < T; base += 64) {          // (uniform: every lane runs every round and every chain step)
        bool shut = false;
        if (by_height) {
            const int steps = min(64, T - base);
            for (int l = 0; l < steps; ++l) {
                const int d = ((base + l) / p.repeat) * p.adim + kCemGripLift;      // < D: its lane stored a value
                const float z0 = __shfl(f[0], d & 63), z1 = __shfl(f[1], d & 63);
                const double step = __dmul_rn((double)(d < 64 ? z0 : z1), g.norm);
                c = base + l == 0 ? step : __dadd_rn(c, step);
                bool below = __dadd_rn(c, g.state_z) < g.z_thresh;
                if (!g.reopen) {
                    latched = latched || below;
                    below = latched;
                }
                if (l == lane) shut = below;
            }
        }
        const int t = base + lane;      // (no shuffle below: the lanes past T may idle)
        if (t < T) {
            if (draws) {
                unsigned w[4];
                cem_philox((unsigned)(t >> 2), kCemGripTrial, (unsigned)i, p.call, p.seed_lo, p.seed_hi, w);
                const int q = t & 3;
                const unsigned word = q == 0 ? w[0] : (q == 1 ? w[1] : (q == 2 ? w[2] : w[3]));
                const double u = __ddiv_rn((double)word, 4294967296.0);
                if (by_height) shut = shut != (u < g.deviation_prob);
                else shut = u < (double)g.share[t];
            }
            out[t * W + p.adim] = shut ? g.close_cmd : g.open_cmd;
        }
    }
    cem_fill_tail(out, lane, T, W, p.adim + 1, p.tail - 1, p.tail_value + 1);    // (behind the gripper column: tail_value[1 ..])
}

}  // namespace vf
