// vf_net_conv.h - the matrix-pipe core the small networks beside the predictor share (vf_frame_scorer.h c2 .. c4,
// vf_registration_net.h d2 .. u3): a 3x3 convolution with zero padding 1 as an implicit GEMM, one wave per task = (image,
// tile of 32 output positions, group of NT * 32 output channels), v_mfma_f32_32x32x2_f32 (exact fp32).  A kernel maps its
// lane to an output position, calls net_conv3x3_mma once and writes its own epilogue.
//
// Same bits everywhere: every output value is ONE fmaf chain whose order depends on the layer alone - taps (ky, kx)
// ascending; inside a tap the input channels in steps of eight, a step's channels in the order 0, 4, 1, 5, 2, 6, 3, 7 (lane
// half h of the MFMA supplies channels 4h .. 4h + 3) - and an MFMA row (an output position) does not see the other rows
// of its tile.  Padding taps and idle rows multiply zeros (fmaf(0, w, acc) == acc), so they change nothing.  K is never
// split.  A value is therefore the same whatever batch, chunk, group, slot, lane or rank computes it, and whatever NT and
// tile shape the launch chose.
//
// Packed weights (pack_conv3x3_mfma in vf_engine_sidenet.inc): canonical [3][3][Cin][Cout] -> [step][half][ceil(Cout / 32)]
// [32][4], step = tap * Cin / 8 + channel block, element q of lane (j, half) = w[tap][8 * block + 4 * half + q][32 * ntile + j]
// (columns past Cout are zero): one 16-byte load of each operand feeds four MFMAs.  MFMA lane layout (lane l: A[i = l & 31]
// [k = l >> 5], B[k = l >> 5][j = l & 31], D register r: row net_mma_row(r, l >> 5), column l & 31) as in vf_fc_tile.h.
#pragma once
#include <hip/hip_runtime.h>
#include "vf_conv_mfma.h"

namespace vf {

constexpr int kNetConvThreads = 256;    // four waves, one task each (launch_net_conv sizes the grid to match)

// the task of this wave: false past the last one (no barrier in these kernels)
__device__ __forceinline__ bool net_conv_task(int n_img, int mtiles, int ngroups, int &img, int &mt, int &ng) {
    const long long task = (long long)blockIdx.x * (kNetConvThreads / 64) + (threadIdx.x >> 6);
    if (task >= (long long)n_img * mtiles * ngroups) return false;
    ng = (int)(task % ngroups);
    mt = (int)((task / ngroups) % mtiles);
    img = (int)(task / ((long long)ngroups * mtiles));
    return true;
}

// the row of the 32-position tile that accumulator register r of lane half `half` holds
__device__ __forceinline__ int net_mma_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// out[nt] = the sums of the tile's 32 positions x output channels 32 * (ng * NT + nt) .. + 31 over all 9 * Cin products.
// Lane (j, half) stands for the position whose tap (ky, kx) reads img[y + ky - 1][x + kx - 1] (img [Hin][Win][Cin], Cin a
// multiple of 8); row_ok = false marks an idle row.  w4: the layer's packed weights, ntile_all = ceil(Cout / 32).
template <int NT>
__device__ __forceinline__ void net_conv3x3_mma(f32x16 (&out)[NT], const float *img, int Hin, int Win, int Cin, int y, int x,
                                                bool row_ok, const f32x4 *w4, int ntile_all, int ng, int j, int half) {
    const int blocks = Cin / 8;
    // (accumulated here and handed over at the end: summed through the reference, the pooled NT = 2 kernel of the
    // registration net takes 84 instead of 76 registers, a wave of occupancy)
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    for (int tap = 0; tap < 9; ++tap) {
        const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
        const bool ok = row_ok && iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
        const f32x4 *a4 = reinterpret_cast<const f32x4 *>(img + ((long long)(ok ? iy : 0) * Win + (ok ? ix : 0)) * Cin + 4 * half);
        const f32x4 *b4 = w4 + ((long long)(tap * blocks * 2 + half) * ntile_all + ng * NT) * 32 + j;
        for (int s = 0; s < blocks; ++s) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (ok) a = a4[2 * s];
            f32x4 bq[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bq[nt] = b4[((long long)s * 2 * ntile_all + nt) * 32];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], bq[nt][q], acc[nt], 0, 0, 0);
        }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) out[nt] = acc[nt];
}

}  // namespace vf
