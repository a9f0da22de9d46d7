// fq_mx_cols.h -- MX block-scaled fake quantization with the blocks running down the columns: the block of a
// contiguous [rows, cols] tensor is the 32 elements (32k .. 32k + 31, c) of one column, which is what a GEMM that contracts over axis 0
// needs (dX = dY W over `out`, dW = dY^T X over the tokens).  Per block the arithmetic is mx_kernel's, through the same helpers of
// fq_mx.h (mx_block_consts, mx_rint, mx_value): the result is the row kernel's on the transposed tensor, bit for bit.
//
// The column tile, in stages that the nearest kernel here and the stochastic one (mx_sr_cols_kernel, fq_mx_sr.h) both call (DESIGN.md
// section 20); each kernel keeps its own loop nest over the loaded tile:
//   mx_cols_load     A workgroup covers MXC_TILE_ROWS = 32 rows (one block of every column) by MXC_TILE_STRIPS = 64 column strips of
//                    16 bytes; each of its four waves holds 16 neighbouring strips.  Lane l of a wave owns strip l & 15 and the 8 rows
//                    (l >> 4) * 8 .. + 7: 8 vectors in flight, and every row segment a wave touches is 256 contiguous bytes (1 KiB for
//                    the workgroup).  A vector holds 16 / esize columns, so a lane carries that many independent blocks; their
//                    absmaxes stay packed as in the row kernels (two 16-bit patterns per dword) and are folded over the lane's 8 rows
//                    in registers.  Strips past the last one re-load the last strip (the tile's rows are always whole: rows is a
//                    multiple of 32); such a lane's partners hold the same strip, so it only ever meets lanes that are not stored
//                    either.  Only stores are predicated (`live`).
//   mx_cols_consts   one dword of the strip: the fold over the four row groups -- lanes l, l ^ 16, l ^ 32, l ^ 48 -- with
//                    v_permlane16_swap and v_permlane32_swap (mx_cols_group_max), then the constants of its one or two columns'
//                    blocks.  The amax never leaves the registers.
//   mx_cols_kernel   one pass, no LDS, no barrier: dword by dword, the constants and then the lane's 8 rows in place.
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

// The lane's place in the tile and its loads.  -> first: the lane's vector of its first row; row i of its RPL rows is first + i * a.ncs.
// A row is ncs whole vectors, so that is also the flat vector index in the contiguous tensor, which the stochastic kernel takes as its
// noise index: the tile geometry may change here and nowhere else.  live <- the lane's strip exists (its rows are stored); w <- the
// lane's RPL vectors as dwords; acc[d] <- the packed absmax of dword d over the lane's rows.
template <int DT, int RPL> __device__ __forceinline__ int64_t mx_cols_load(const MxColsArgs& a, uint32_t (&w)[RPL][4], uint32_t (&acc)[4], bool& live) {
    using T = Ty<DT>;
    static_assert(RPL * MXC_ROW_GROUPS == MXC_TILE_ROWS, "the wave's row groups share the tile's rows");
    const uint32_t rt = blockIdx.x / a.nct, ct = blockIdx.x - rt * a.nct;   // column tiles of one row tile follow one another
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const int64_t strip = (int64_t)ct * MXC_TILE_STRIPS + wave * MXC_WAVE_STRIPS + (lane & (MXC_WAVE_STRIPS - 1));
    const int64_t row = (int64_t)rt * MXC_TILE_ROWS + (lane / MXC_WAVE_STRIPS) * RPL;
    live = strip < a.ncs;
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
#pragma unroll
    for (int d = 0; d < 4; ++d) acc[d] = 0u;
#pragma unroll
    for (int i = 0; i < RPL; ++i) {
        w[i][0] = r[i].x, w[i][1] = r[i].y, w[i][2] = r[i].z, w[i][3] = r[i].w;
#pragma unroll
        for (int d = 0; d < 4; ++d) acc[d] = T::absmax_acc(acc[d], w[i][d]);
    }
    return first;
}

// accd: mx_cols_load's acc of one dword of the strip -> mx_block_consts of its EPD columns' blocks
template <int DT, bool CEIL>
__device__ __forceinline__ void mx_cols_consts(uint32_t accd, const MxFmt& f, bool* bad, int* nE, int* yk, float* maxx) {
    using T = Ty<DT>;
    const uint32_t m = mx_cols_group_max<DT>(accd);   // the patterns of the columns' amax
#pragma unroll
    for (int k = 0; k < T::EPD; ++k)
        mx_block_consts<CEIL>(T::EPD == 1 ? m : T::absmax_finish(k ? m >> 16 : m & 0xFFFFu), f, bad[k], nE[k], yk[k], maxx[k]);
}

template <int DT, bool CEIL>
__global__ __launch_bounds__(MX_TPB) void mx_cols_kernel(MxColsArgs a, MxFmt f) {
    using T = Ty<DT>;
    constexpr int RPL = MXC_TILE_ROWS / MXC_ROW_GROUPS;   // rows per lane
    uint32_t w[RPL][4], acc[4];
    bool live;
    const int64_t first = mx_cols_load<DT, RPL>(a, w, acc, live);

    const int bmin = f.emin + 127;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        bool bad[T::EPD];
        int nE[T::EPD], yk[T::EPD];
        float maxx[T::EPD];
        mx_cols_consts<DT, CEIL>(acc[d], f, bad, nE, yk, maxx);
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
