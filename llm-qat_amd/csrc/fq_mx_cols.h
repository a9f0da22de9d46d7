// fq_mx_cols.h -- MX block-scaled fake quantization with the blocks running down the columns: the block of a
// contiguous [rows, cols] tensor is the 32 elements (32k .. 32k + 31, c) of one column, which is what a GEMM that contracts over axis 0
// needs (dX = dY W over `out`, dW = dY^T X over the tokens).  Per block the arithmetic is mx_kernel's, through the same helpers of
// fq_mx.h (mx_shared_exp / mx_shared_exp_ceil, mx_rint, mx_value): the result is the row kernel's on the transposed tensor, bit for bit.
//
//   mx_cols_kernel   one pass, no LDS, no barrier.  A workgroup covers MXC_TILE_ROWS = 32 rows (one block of every column) by
//                    MXC_TILE_STRIPS = 64 column strips of 16 bytes; each of its four waves holds 16 neighbouring strips.  Lane l of a wave owns
//                    strip l & 15 and the 8 rows (l >> 4) * 8 .. + 7: 8 vectors in flight, and every row segment a wave touches is 256
//                    contiguous bytes (1 KiB for the workgroup).  A vector holds 16 / esize columns, so a lane carries that many
//                    independent blocks; their absmaxes stay packed as in the row kernels (two 16-bit patterns per dword), are folded
//                    over the lane's 8 rows in registers and over the four row groups -- lanes l, l ^ 16, l ^ 32, l ^ 48 -- with
//                    v_permlane16_swap and v_permlane32_swap.  The amax never leaves the registers.
// Strips past the last one re-load the last strip (the tile's rows are always whole: rows is a multiple of 32); such a lane's partners hold
// the same strip, so it only ever meets lanes that are not stored either.  Only stores are predicated.
#pragma once
#include "fq_mx.h"

namespace fq {

static_assert(MX_TPB == 64 * (MXC_TILE_STRIPS / MXC_WAVE_STRIPS), "one wave per MXC_WAVE_STRIPS strips of the tile");
static_assert(MXC_WAVE_STRIPS * MXC_ROW_GROUPS == 64 && MXC_WAVE_STRIPS == 16 && MXC_ROW_GROUPS == 4, "row groups are the wave's four DPP rows");
static_assert(MXC_TILE_ROWS == 32, "a tile holds one MX block of every column");

// max of the packed |x| patterns over the wave's four row groups: each swap hands a lane its own value and its partner's (l ^ 16: odd
// rows of the first operand trade places with even rows of the second; l ^ 32: the same with the wave's halves)
template <int DT> __device__ __forceinline__ uint32_t mx_cols_group_max(uint32_t v) {
    using T = Ty<DT>;
    const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    v = T::absmax_acc(p[0], p[1]);
    const auto q = __builtin_amdgcn_permlane32_swap(v, v, false, false);
    return T::absmax_acc(q[0], q[1]);
}

template <int DT, bool CEIL>
__global__ __launch_bounds__(MX_TPB) void mx_cols_kernel(MxColsArgs a, MxFmt f) {
    using T = Ty<DT>;
    constexpr int RPL = MXC_TILE_ROWS / MXC_ROW_GROUPS;   // rows per lane
    const uint32_t rt = blockIdx.x / a.nct, ct = blockIdx.x - rt * a.nct;   // column tiles of one row tile follow one another
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int64_t strip = (int64_t)ct * MXC_TILE_STRIPS + wave * MXC_WAVE_STRIPS + (lane & (MXC_WAVE_STRIPS - 1));
    const int64_t row = (int64_t)rt * MXC_TILE_ROWS + (lane / MXC_WAVE_STRIPS) * RPL;
    const bool live = strip < a.ncs;
    const int64_t first = row * a.ncs + (live ? strip : a.ncs - 1);
    const uint4* __restrict__ xv = (const uint4*)a.x;

    uint4 r[RPL];
    if (a.ntl) {
#pragma unroll
        for (int i = 0; i < RPL; ++i) r[i] = ld16<true>(&xv[first + i * a.ncs]);
    } else {
#pragma unroll
        for (int i = 0; i < RPL; ++i) r[i] = ld16<false>(&xv[first + i * a.ncs]);
    }

    uint32_t w[RPL][4], acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        w[i][0] = r[i].x, w[i][1] = r[i].y, w[i][2] = r[i].z, w[i][3] = r[i].w;
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[d] = T::absmax_acc(acc[d], w[i][d]);
    }

    const int bmin = f.emin + 127;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t m = mx_cols_group_max<DT>(acc[d]);   // dword d of the strip: the patterns of its EPD columns' amax
        int nE[T::EPD], yk[T::EPD];
        float maxx[T::EPD];
        bool bad[T::EPD];
#pragma unroll
        for (int k = 0; k < T::EPD; ++k) {
            const uint32_t ab = T::EPD == 1 ? m : T::absmax_finish(k ? m >> 16 : m & 0xFFFFu);   // fp32 bits of the block's amax
            bad[k] = ab >= 0x7F800000u;                                                          // a NaN or Inf in the block
            const int E = CEIL ? mx_shared_exp_ceil(ab, f.emax, f.maxnorm) : mx_shared_exp(ab, f.emax);
            nE[k] = -E, yk[k] = E - 127 - f.mbits;
            maxx[k] = __builtin_amdgcn_ldexpf(f.maxnorm, E);
        }
#pragma unroll
        for (int i = 0; i < RPL; ++i) {
            float fd[T::EPD];
            T::unpack(w[i][d], fd);
#pragma unroll
            for (int k = 0; k < T::EPD; ++k) {
                int sb;
                const float rr = mx_rint(fd[k], nE[k], bmin, f.mbits, sb);
                fd[k] = bad[k] ? as_f(0x7FC00000u) : mx_value(fd[k], rr, sb, yk[k], maxx[k]);
            }
            w[i][d] = T::pack(fd);
        }
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < RPL; ++i) st16<true>(&((uint4*)a.y)[first + i * a.ncs], make_uint4(w[i][0], w[i][1], w[i][2], w[i][3]));
    }
}

// a and f validated by fqt_mx_fwd_cols (fq_api.hip): whole 32-row tiles, ncs > 0, row_tiles * a.nct within one launch's grid
template <int DT> int launch_mx_cols(bool ceil, MxColsArgs a, MxFmt f, int64_t row_tiles, hipStream_t st) {
    begin_launches();
    const dim3 grid((unsigned)(row_tiles * a.nct));
    if (ceil) launch(mx_cols_kernel<DT, true>, grid, dim3(MX_TPB), st, a, f);
    else launch(mx_cols_kernel<DT, false>, grid, dim3(MX_TPB), st, a, f);
    return launch_result();
}

#define FQ_INSTANTIATE_MX_COLS(DT) template int launch_mx_cols<DT>(bool, MxColsArgs, MxFmt, int64_t, hipStream_t);

}  // namespace fq
