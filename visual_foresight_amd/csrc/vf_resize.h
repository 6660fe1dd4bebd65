// vf_resize.h - exact area average for shrinking NHWC images on the device (reference visual_mpc/utils/im_utils.py:6-15:
// cv2.resize(..., INTER_AREA) of every observation; goal_im_controller.py:89; register_gtruth_controller.py:44-51).
//
// Specification (this project's own; parity with OpenCV's INTER_AREA is unpinned).  Per axis the weights
// are integers: destination row i covers [i*Hs, (i+1)*Hs) and source row r covers [r*Hd, (r+1)*Hd) of one common axis of
// length Hs*Hd; wy[i][r] is the length of their overlap, sum_r wy = Hs; wx likewise, sum_c wx = Ws; A = Hs*Ws is the total
// weight of every output.
//   uint8    S = sum_r sum_c wy*wx*v is an exact integer (Hs*Ws <= 2^22: below 2^30); out = S / A rounded half to even in
//            integer arithmetic.
//   float32  one float64 sum per output element: source rows ascending, columns ascending within a row, every term
//            (double)(wy*wx) * (double)v (exact), additions rounded to nearest, never contracted; one float64 division by
//            A, one rounding to float32.  An image's output depends on that image and the two sizes alone.  Equal sizes
//            give a copy of the VALUES, not of the bits: the sum starts at +0.0, so -0.0 comes back as +0.0 (and a NaN
//            as some NaN); uint8 is copied exactly.
//
//   resize_int_kernel   integer ratios (Hs % Hd == 0 and Wd divides Ws): the footprints tile the source, every source
//                       element is read once, straight from global memory.  A destination pixel's footprint is walked
//                       row segment by row segment (fx * C contiguous elements each): by one thread for float32,
//                       whose order of additions is the specification; by `split` neighbouring lanes for uint8 (lane q
//                       takes rows q, q + split, ...), whose integer sums are then combined with wavefront shuffles.
//   resize_frac_kernel  any other ratio: footprints of neighbouring outputs share source rows and columns, so the band's
//                       source rows are staged in LDS once (when they fit; otherwise the same arithmetic reads global
//                       memory).  One thread per destination element.
// Both: one workgroup per (image, band of destination rows).  A contiguous piece of source is read with 16-byte loads
// from its first 16-byte boundary on, with scalar loads in front of that and behind the last whole 16 bytes, so any base
// and any row pitch is served.  What "a piece" is differs: resize_frac_kernel stages the band's rows as ONE piece - with an
// aligned base and pitch that is all 16-byte loads.  resize_int_kernel reads SEGMENT-WISE: a piece is one pixel's row
// segment of fx * C elements (6 bytes for uint8 x 3 at factor 2, 30 at factor 10, 24 for float32 x 3 at factor 2), its
// alignment is decided per segment, and most of that path therefore runs on scalar byte / dword loads; only segments of
// at least 16 bytes see a 16-byte load at all.  No atomics, static LDS only, plain vector stores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "vf_conv_mfma.h"

namespace vf {

constexpr int kResizeThreads = 256;
constexpr int kResizeStageBytes = 48 * 1024;        // static LDS of resize_frac_kernel
constexpr long long kResizeMaxArea = 1LL << 22;     // Hs * Ws: keeps the uint8 sum below 2^30
constexpr int kResizeMaxSplit = 16;                 // most lanes per destination pixel (resize_int_kernel, uint8)
static_assert(64 % kResizeMaxSplit == 0 && (kResizeMaxSplit & (kResizeMaxSplit - 1)) == 0,
              "the lanes of a pixel are one aligned group inside a wave: the shuffles never cross a wave");

struct ResizeParams {
    const void *src;
    void *dst;
    int Hs, Ws, C, Hd, Wd;
    int band;               // destination rows per workgroup
    int n_bands;            // ceil(Hd / band)
    int stage;              // resize_frac_kernel: 1 = the band's source rows fit the LDS stage
    int split;              // resize_int_kernel: lanes per destination pixel - a power of two, at most kResizeMaxSplit and at
                            // most the row factor Hs / Hd, chosen by the launcher; uint8 only, 1 for float32
};

template <class T> struct ResizeAcc;
template <> struct ResizeAcc<uint8_t> {
    unsigned s;
    __device__ __forceinline__ void zero() { s = 0u; }
    __device__ __forceinline__ void add(int w, uint8_t v) { s += (unsigned)w * (unsigned)v; }
    __device__ __forceinline__ uint8_t finish(int area) const {
        const unsigned A = (unsigned)area;
        unsigned q = s / A;
        const unsigned rem = s - q * A;
        q += (2u * rem > A) || (2u * rem == A && (q & 1u));
        return (uint8_t)q;
    }
};
template <> struct ResizeAcc<float> {
    double s;
    __device__ __forceinline__ void zero() { s = 0.0; }
    __device__ __forceinline__ void add(int w, float v) { s = __dadd_rn(s, __dmul_rn((double)w, (double)v)); }
    __device__ __forceinline__ float finish(int area) const { return (float)__ddiv_rn(s, (double)area); }
};

__device__ __forceinline__ void resize_unpack(const uint4 &q, uint8_t *out) {
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}
__device__ __forceinline__ void resize_unpack(const uint4 &q, float *out) {
    out[0] = __uint_as_float(q.x); out[1] = __uint_as_float(q.y);
    out[2] = __uint_as_float(q.z); out[3] = __uint_as_float(q.w);
}

// f(k, p[k]) for k = 0 .. len-1 in ascending order: scalar loads up to the first 16-byte boundary, 16-byte loads, scalar tail
template <class T, class F> __device__ __forceinline__ void resize_walk(const T *p, int len, F f) {
    constexpr int kPer = 16 / (int)sizeof(T);
    int k = 0;
    for (; k < len && (reinterpret_cast<uintptr_t>(p + k) & 15); ++k) f(k, p[k]);
    for (; k + kPer <= len; k += kPer) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p + k);
        T v[kPer];
        resize_unpack(q, v);
#pragma unroll
        for (int j = 0; j < kPer; ++j) f(k + j, v[j]);
    }
    for (; k < len; ++k) f(k, p[k]);
}

// Integer ratios fy = Hs / Hd, fx = Ws / Wd: every weight is Hd * Wd.  Grid n * n_bands; p.split lanes -> one destination
// pixel of the band, kResizeThreads / p.split pixels per sweep.  Element k of a row segment belongs to channel k % C (a
// segment starts at a pixel).  The sweep count is the same for every lane, so all of a wave reach the shuffles.
template <class T, int C>
VF_GLOBAL VF_LAUNCH_BOUNDS(kResizeThreads) void resize_int_kernel(const ResizeParams p) {
    const int img = blockIdx.x / p.n_bands, band = blockIdx.x % p.n_bands;
    const int i0 = band * p.band, i1 = min(i0 + p.band, p.Hd);
    const int fy = p.Hs / p.Hd, fx = p.Ws / p.Wd, w = p.Hd * p.Wd, area = p.Hs * p.Ws;
    const long long row_elems = (long long)p.Ws * C;
    const T *src = static_cast<const T *>(p.src) + (long long)img * p.Hs * row_elems;
    T *dst = static_cast<T *>(p.dst) + (long long)img * p.Hd * p.Wd * C;
    const int n_pix = (i1 - i0) * p.Wd;
    const int R = p.split, q = threadIdx.x & (R - 1), per_sweep = kResizeThreads / R;
    for (int e0 = 0; e0 < n_pix; e0 += per_sweep) {
        const int e = e0 + threadIdx.x / R;
        const bool live = e < n_pix;
        const int i = i0 + (live ? e : 0) / p.Wd, j = (live ? e : 0) % p.Wd;
        ResizeAcc<T> acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c].zero();
        for (int r = i * fy + q; live && r < (i + 1) * fy; r += R) {
            int ch = 0;
            resize_walk<T>(src + r * row_elems + (long long)j * fx * C, fx * C, [&](int, T v) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (c == ch) acc[c].add(w, v);
                ch = (ch + 1 == C) ? 0 : ch + 1;
            });
        }
        if constexpr (std::is_same<T, uint8_t>::value) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                for (int m = R >> 1; m > 0; m >>= 1) acc[c].s += (unsigned)__shfl_xor((int)acc[c].s, m);
        }
        if (live && q == 0) {
            T *o = dst + ((long long)i * p.Wd + j) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = acc[c].finish(area);
        }
    }
}

// Any ratio.  The band's source rows [r_lo, r_hi) are one contiguous piece of the image; with p.stage it is copied to
// LDS at the same offset from a 16-byte boundary as it has in memory, so the 16-byte loads and stores line up.
template <class T>
VF_GLOBAL VF_LAUNCH_BOUNDS(kResizeThreads) void resize_frac_kernel(const ResizeParams p) {
    __shared__ uint4 s_stage[kResizeStageBytes / 16];
    const int img = blockIdx.x / p.n_bands, band = blockIdx.x % p.n_bands, tid = threadIdx.x;
    const int i0 = band * p.band, i1 = min(i0 + p.band, p.Hd);
    const int C = p.C, area = p.Hs * p.Ws;
    const long long row_elems = (long long)p.Ws * C;
    const int r_lo = (int)(((long long)i0 * p.Hs) / p.Hd);
    const int r_hi = (int)(((long long)i1 * p.Hs + p.Hd - 1) / p.Hd);
    const T *g = static_cast<const T *>(p.src) + ((long long)img * p.Hs + r_lo) * row_elems;
    T *dst = static_cast<T *>(p.dst) + (long long)img * p.Hd * p.Wd * C;
    const T *rows = g;
    if (p.stage) {
        const int n_elems = (int)((r_hi - r_lo) * row_elems);
        const int shift = (int)((reinterpret_cast<uintptr_t>(g) & 15) / sizeof(T));
        T *s = reinterpret_cast<T *>(s_stage) + shift;
        constexpr int kPer = 16 / (int)sizeof(T);
        const int head = min(n_elems, (kPer - shift) % kPer);
        const int n16 = (n_elems - head) / kPer;
        if (tid < head) s[tid] = g[tid];
        const uint4 *g16 = reinterpret_cast<const uint4 *>(g + head);
        uint4 *s16 = reinterpret_cast<uint4 *>(s + head);
        for (int k = tid; k < n16; k += kResizeThreads) s16[k] = g16[k];
        for (int k = head + n16 * kPer + tid; k < n_elems; k += kResizeThreads) s[k] = g[k];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        rows = s;
    }
    const int n_out = (i1 - i0) * p.Wd * C;
    for (int e = tid; e < n_out; e += kResizeThreads) {
        const int c = e % C, j = (e / C) % p.Wd, i = i0 + e / (C * p.Wd);
        const long long y0 = (long long)i * p.Hs, y1 = y0 + p.Hs, x0 = (long long)j * p.Ws, x1 = x0 + p.Ws;
        const int ra = (int)(y0 / p.Hd), rb = (int)((y1 + p.Hd - 1) / p.Hd);
        const int ca = (int)(x0 / p.Wd), cb = (int)((x1 + p.Wd - 1) / p.Wd);
        ResizeAcc<T> acc;
        acc.zero();
        for (int r = ra; r < rb; ++r) {
            const long long ry = (long long)r * p.Hd;
            const int wy = (int)(min(y1, ry + p.Hd) - max(y0, ry));
            const T *row = rows + (r - r_lo) * row_elems + c;
            for (int cc = ca; cc < cb; ++cc) {
                const long long cx = (long long)cc * p.Wd;
                const int wx = (int)(min(x1, cx + p.Wd) - max(x0, cx));
                acc.add(wy * wx, row[(long long)cc * C]);
            }
        }
        dst[((long long)i * p.Wd + j) * C + c] = acc.finish(area);
    }
}

}  // namespace vf
