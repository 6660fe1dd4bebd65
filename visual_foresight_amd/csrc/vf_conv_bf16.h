// vf_conv_bf16.h - conv-LSTM gate tile in plain bf16: one bf16 MFMA product per multiply, fp32 accumulation.
//
// Opt-in precision mode (vf_config.precision = 2).  It is the a1 b1 term of the split-bf16 tile (vf_conv_bf16x6.h) alone:
// the staged activation (LayerNorm + relu of the producer applied as there) is rounded ONCE, to nearest even, into ONE bf16
// plane, and the weights are rounded once on the host (pack_weights_bf16 in vf_engine.hip).  Every bf16 x bf16 product is
// exact in fp32 and the MFMA accumulates in fp32, so the only error beyond an fp32 dot product is the operand rounding
// (2^-9 relative per operand) - the accuracy class of a half-precision predictor, not of the other two modes.  Bias, gate
// math, cell state and LayerNorm statistics are the shared fp32 epilogue (conv_epilogue<4, EPI_LSTM, 1>).
//
// Structure = the G == 4, 128-row tile of vf_conv_bf16x6.h with a K loop built for 4 MFMAs per tap instead of 24:
//  * the A plane is [pixel][kBf1KC + 8 pad] bf16 (rows of 48 B at 16 channels, 80 B at 32: the 16-lane groups of
//    ds_read_b128 hit 16 distinct 16-B slots either way);
//  * a BARRIER COVERS A KERNEL ROW of one 16-channel k-step: 5 taps x 4 gates = 20 MFMAs.  The weights of a row are one
//    contiguous 20 KiB block, packed [chunk16][ky][cg][kx][gate][k-half][32 columns][8 channels]; the workgroup fetches the
//    next row's block while it multiplies this one (five raw buffer loads per thread) and parks it in the other LDS buffer;
//  * a chunk of kBf1KC channels is staged per pass over the haloed tile.  The summation order - chunk16, ky, kx, k - does not
//    depend on kBf1KC, so the chunk size changes time only, never bits.
// Every barrier of the K loop is preceded by an explicit LDS wait (tools/lint_barriers.py).
#pragma once
#include <hip/hip_runtime.h>
#include "vf_conv_bf16x6.h"

namespace vf {

#ifndef VF_BF16_KC
#define VF_BF16_KC 32       // measured against 16: see the comment in front of the kernel
#endif
constexpr int kBf1KC = VF_BF16_KC;              // channels per staged chunk: 16 or 32
constexpr int kBf1KS = kBf1KC / 16;             // MFMA k-steps per chunk
constexpr int kBf1RowUnits = kBf1KC / 8 + 1;    // 16-B units per pixel row of the plane (8 channels of padding)
constexpr int kBf1KW = 5;                       // taps per kernel row (every conv-LSTM of the engine is 5 x 5)
constexpr int kBf1StageUnits = kBf1KW * 4 * 64; // 16-B units of one weight stage: [kx][gate][64 lanes] = 20 KiB
static_assert(kBf1KC == 16 || kBf1KC == 32, "the plane is staged in chunks of 16 or 32 channels");
static_assert(kBf1StageUnits % kConvThreads == 0, "every thread fetches the same number of weight units per stage");

// LDS bytes of the tile for a layer geometry (host + device)
__host__ __device__ inline size_t bf16_lds_bytes(int NI, int LH, int LW) {
    return (size_t)NI * LH * LW * kBf1RowUnits * 16 + ((size_t)4 * NI + 16) * 4 + (size_t)2 * kBf1StageUnits * 16;
}

template <int MREP, class PT>
__device__ __forceinline__ void conv_lstm_bf16_tile(const PT &p, const int bx_, const int by_, float *smem) {
    const int bx = __builtin_amdgcn_readfirstlane(bx_), by = __builtin_amdgcn_readfirstlane(by_);   // (see conv_tile)
    static_assert(MREP == 1, "128-row tiles (one row block per wave)");
    constexpr int G = 4;
    constexpr int WROWS = MREP * 32;
    constexpr int kFetch = kBf1StageUnits / kConvThreads;           // weight units per thread and stage
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, kh = lane >> 5;
    const int LH = (p.TH - 1) * p.stride + p.KH, LW = (p.TW - 1) * p.stride + p.KW;
    const int tile_px = LH * LW;
    const int plane_units = p.NI * tile_px * kBf1RowUnits;
    u16x8 *aP = reinterpret_cast<u16x8 *>(smem);                    // [pixel][kBf1RowUnits]
    float *lnTab = smem + (size_t)plane_units * 4;                  // [2][NI][2]
    long long *red = reinterpret_cast<long long *>(lnTab + 4 * p.NI);
    u16x8 *bsm = reinterpret_cast<u16x8 *>(lnTab + 4 * p.NI + 16);  // [2 buf][kx][gate][64]
    const int cg = by;
    const int tiles_per_img = p.tilesY * p.tilesX;

    int bimg0, ty0, tx0;
    if (p.NI == 1) {
        bimg0 = bx / tiles_per_img;
        const int tile_id = bx % tiles_per_img;
        ty0 = (tile_id / p.tilesX) * p.TH;
        tx0 = (tile_id % p.tilesX) * p.TW;
    } else {
        bimg0 = bx * p.NI; ty0 = 0; tx0 = 0;
    }

    const bool late = p.late_cnt != nullptr;     // early-started item: see ConvParams::late_cnt
    ln_table(p, bimg0, lnTab, 0, late ? 1 : 2);

    const int px_per_img = p.TH * p.TW;
    int abase;                          // 16-B unit of this lane's row inside the plane (+ k-half)
    {
        const int row = wave * WROWS + n;
        const int img = row / p.RPI, rem = row % p.RPI;
        const bool ok = img < p.NI && rem < px_per_img;
        const int y = rem / p.TW, x = rem % p.TW;
        abase = (ok ? (img * tile_px + y * p.stride * LW + x * p.stride) * kBf1RowUnits : 0) + kh;
    }

    f32x16 acc[MREP][G];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][g][r] = 0.f;

    const int total_chunks = p.seg[0].nchunk + (p.nseg > 1 ? p.seg[1].nchunk : 0);
    const int nst = total_chunks * kBf1KS * p.KH;                   // weight stages: (chunk16, ky)
    const unsigned w_loff = (unsigned)((cg * kBf1StageUnits + tid) * 16);      // this thread's first unit of a stage
    const unsigned w_stage_b = (unsigned)(p.ncg * kBf1StageUnits * 16);        // bytes per (chunk16, ky)
    const __amdgpu_buffer_rsrc_t w_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(p.Wp16), 0, 0x7FFFFFFF, 0x00020000);
    u16x8 breg[kFetch];
#pragma unroll
    for (int i = 0; i < kFetch; ++i)
        breg[i] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_loff, (unsigned)i * (kConvThreads * 16u), 0));

    const int items = p.NI * tile_px * (kBf1KC / 8);    // (pixel, 8-channel octet) pairs

    for (int ci = 0; ci < total_chunks; ++ci) {
        const int s = (ci < p.seg[0].nchunk) ? 0 : 1;
        const auto &sg = p.seg[s];
        const int c0 = (s == 0 ? ci : ci - p.seg[0].nchunk) * kBf1KC;

        if (late && ci == p.seg[0].nchunk) {         // the recurrent chunks are done: now the layer input is needed
            const int b1 = p.NI == 1 ? bimg0 + 1 : min(bimg0 + p.NI, p.B);
            if (!late_wait(p, bimg0, b1, reinterpret_cast<int *>(red))) return;
            ln_table(p, bimg0, lnTab, 1, 2);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (!std::is_same<PT, ConvParams>::value) VF_TRACE_EVT(TR_STAGE);
        for (int it = tid; it < items; it += kConvThreads) {
            const int pix = it / (kBf1KC / 8), oct = it % (kBf1KC / 8);
            const int img = pix / tile_px, r = pix - img * tile_px;
            const int ly = r / LW, lx = r - ly * LW;
            const int iy = ty0 * p.stride - p.pad + ly, ix = tx0 * p.stride - p.pad + lx;
            const int b = bimg0 + img;
            const int c = c0 + 8 * oct;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = 0.f;
            if (b < p.B && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win && c < sg.C) {
                const float *src = sg.ptr + (long long)b * sg.bstride + ((long long)iy * p.Win + ix) * sg.C + c;
                const f32x4 lo = *reinterpret_cast<const f32x4 *>(src);
                const f32x4 hi = *reinterpret_cast<const f32x4 *>(src + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { v[j] = lo[j]; v[4 + j] = hi[j]; }
                if (sg.ln_part) {
                    const float mean = lnTab[2 * (s * p.NI + img)];
                    const float rstd = lnTab[2 * (s * p.NI + img) + 1];
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int cc = (c + j) % sg.gamma_mod;
                        v[j] = fmaf((v[j] - mean) * rstd, sg.gamma[cc], sg.beta[cc]);
                    }
                }
                if (sg.relu) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
                }
            }
            bf16x8 q;
#pragma unroll
            for (int j = 0; j < 8; ++j) q[j] = (__bf16)v[j];        // the mode's ONE rounding of an activation (RNE)
            aP[pix * kBf1RowUnits + oct] = __builtin_bit_cast(u16x8, q);
        }
        if (ci == 0) {
#pragma unroll
            for (int i = 0; i < kFetch; ++i) bsm[i * kConvThreads + tid] = breg[i];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
        if constexpr (!std::is_same<PT, ConvParams>::value) {
            if (ci == 0) VF_TRACE_EVT(TR_MFMAS, (unsigned long long)(p.KH * kBf1KW * G * MREP));
            VF_TRACE_EVT(TR_KLOOP);
        }

        // ---- K loop: one barrier per kernel row of a k-step.  The next stage's weights are requested first (raw buffer
        // loads: lane offset in one VGPR, stage offset in an SGPR), the five A fragments of the row come through one address
        // register plus immediates, and the twenty B fragments are read tap by tap between the MFMAs.
        for (int ks = 0; ks < kBf1KS; ++ks) {
            for (int ky = 0; ky < p.KH; ++ky) {
                const int st = (ci * kBf1KS + ks) * p.KH + ky;
                const int buf = st & 1;
                const bool more = st + 1 < nst;
                if (more) {
                    const unsigned so = (unsigned)(st + 1) * w_stage_b;
#pragma unroll
                    for (int i = 0; i < kFetch; ++i)
                        breg[i] = __builtin_bit_cast(u16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_loff, so + (unsigned)i * (kConvThreads * 16u), 0));
                }
                const u16x8 *arow = aP + abase + ky * LW * kBf1RowUnits + ks * 2;
                const u16x8 *brow = bsm + buf * kBf1StageUnits + lane;
                bf16x8 a[kBf1KW];
#pragma unroll
                for (int kx = 0; kx < kBf1KW; ++kx) a[kx] = __builtin_bit_cast(bf16x8, arow[kx * kBf1RowUnits]);
#pragma unroll
                for (int kx = 0; kx < kBf1KW; ++kx) {
                    bf16x8 bw[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) bw[g] = __builtin_bit_cast(bf16x8, brow[(kx * G + g) * 64]);
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        acc[0][g] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[kx], bw[g], acc[0][g], 0, 0, 0);
                }
                if (more) {
                    u16x8 *bw_ = bsm + (buf ^ 1) * kBf1StageUnits + tid;
#pragma unroll
                    for (int i = 0; i < kFetch; ++i) bw_[i * kConvThreads] = breg[i];
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __syncthreads();
            }
        }
    }
    if constexpr (!std::is_same<PT, ConvParams>::value) VF_TRACE_EVT(TR_EPI);
    conv_epilogue<G, EPI_LSTM, MREP>(p, acc, bx, by, 0, red);
}

// Measured (one box, the three precision modes interleaved in one process, device time of the persistent launch;
// profiles/bf16_mode.txt): C2 17.94 ms against 40.45 for the split-bf16 tile and 57.36 for exact fp32; 25 samples 5.89 / 11.24 /
// 10.75; C5 shard on arch 1 100.80 / 189.44 / 242.54.  Staged chunk: 32 channels 17.94 / 5.89 / 100.80 ms against 16 channels
// 18.10 / 5.95 / 101.15 (same bits); 48 does not divide the 32- / 64- / 128-channel segments of the layer table - a third to a
// half of its k-steps would multiply zero padding - and was not built.  159 VGPRs, no spill, stand-alone and out of line.
template <int MREP>
VF_GLOBAL VF_LAUNCH_BOUNDS(kConvThreads, 2) void conv_lstm_bf16_kernel(const ConvParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    conv_lstm_bf16_tile<MREP>(p, blockIdx.x, blockIdx.y, smem);
}

}  // namespace vf
