// fq_shapes.h -- the launch-shape tables of the row kernels: which (threads per row, vectors per thread) instantiation serves a row of
// nvec 16-byte vectors.  Plain C++ (nothing from HIP), so a host program can read the tables the launch layer uses
// (tests/c_host/shape_tables.cpp prints them; tests/test_shape_tables_cpu.py compares the tests' Python mirrors with that).
#pragma once
#include <cstdint>
#include <type_traits>

namespace fq {

constexpr int64_t REG_MAX_VEC = 1024 * 8;    // longest row (in 16-byte vectors) the register kernels hold

// ---- run-time choices -> template arguments: the callable receives std::integral_constant values and reads them as constants ----
template <int V> using Const = std::integral_constant<int, V>;
// a count of 16-byte vectors (or 8-byte half-vectors) per thread, 1 .. 8, as the backward kernels and the fp32-result forward take it
template <class F> inline void by_count(int n, F&& f) {
    switch (n) {
        case 1: f(Const<1>{}); break;
        case 2: f(Const<2>{}); break;
        case 3: f(Const<3>{}); break;
        case 4: f(Const<4>{}); break;
        case 5: f(Const<5>{}); break;
        case 6: f(Const<6>{}); break;
        case 7: f(Const<7>{}); break;
        case 8: f(Const<8>{}); break;
        default: break;
    }
}
// Launch shape of the register-resident row kernels (forward and export) for a row of nvec 16-byte vectors (nvec <= REG_MAX_VEC):
// f(threads per row, vectors per thread), the smallest rung that holds the row.  5 and 7 vectors per thread run as 6 and 8 (no model
// width lands there; why these rungs: the comment above launch_reg in fq_dtype_impl.h).
template <class F> inline void by_reg_shape(int64_t nvec, F&& f) {
    if (nvec <= 64) f(Const<64>{}, Const<1>{});
    else if (nvec <= 128) f(Const<64>{}, Const<2>{});
    else if (nvec <= 192) f(Const<64>{}, Const<3>{});
    else if (nvec <= 256) f(Const<128>{}, Const<2>{});
    else if (nvec <= 384) f(Const<128>{}, Const<3>{});
    else if (nvec <= 512) f(Const<256>{}, Const<2>{});
    else if (nvec <= 768) f(Const<256>{}, Const<3>{});
    else if (nvec <= 1024) f(Const<512>{}, Const<2>{});
    else if (nvec <= 1536) f(Const<512>{}, Const<3>{});
    else if (nvec <= 2048) f(Const<512>{}, Const<4>{});
    else if (nvec <= 3072) f(Const<512>{}, Const<6>{});
    else if (nvec <= 4096) f(Const<512>{}, Const<8>{});
    else if (nvec <= 6144) f(Const<1024>{}, Const<6>{});
    else f(Const<1024>{}, Const<8>{});
}
// Launch shapes of the group-wise kernel (fq_group.h): the (threads per row, vectors per thread) of by_reg_shape for the model widths
// (bf16 4096 -> 256 x 2, 5120 -> 256 x 3, 11008 -> 512 x 3, 13824 -> 512 x 4), fewer in between and a ladder of its own: every rung must
// hold whole groups (TPR * VPT a multiple of 64 vectors, nvec <= TPR * VPT), which 64 x 3, 128 x 3, 512 x 6 and 1024 x 6 do not for gv = 64.
template <class F> inline void by_group_shape(int64_t nvec, F&& f) {
    if (nvec <= 64) f(Const<64>{}, Const<1>{});
    else if (nvec <= 128) f(Const<64>{}, Const<2>{});
    else if (nvec <= 256) f(Const<128>{}, Const<2>{});
    else if (nvec <= 512) f(Const<256>{}, Const<2>{});
    else if (nvec <= 768) f(Const<256>{}, Const<3>{});
    else if (nvec <= 1024) f(Const<512>{}, Const<2>{});
    else if (nvec <= 1536) f(Const<512>{}, Const<3>{});
    else if (nvec <= 2048) f(Const<512>{}, Const<4>{});
    else if (nvec <= 4096) f(Const<1024>{}, Const<4>{});
    else f(Const<1024>{}, Const<8>{});
}


// Tile of the column-block MX kernel (fq_mx_cols.h): a workgroup covers MXC_TILE_ROWS rows (one MX block down every column) by
// MXC_TILE_STRIPS 16-byte column strips (16 / esize columns each); a wave holds MXC_WAVE_STRIPS of the strips, its MXC_ROW_GROUPS
// quarter-waves MXC_TILE_ROWS / MXC_ROW_GROUPS rows each.  tests/test_gpu_mx_cols.py reads these four lines.
constexpr int MXC_TILE_ROWS = 32;
constexpr int MXC_TILE_STRIPS = 64;
constexpr int MXC_WAVE_STRIPS = 16;
constexpr int MXC_ROW_GROUPS = 4;

// Work split of the decode attention (fq_attn_decode.h): a wave walks the keys in tiles of DEC_TILE (two 16-key score tiles, the k of one
// PV matrix instruction), a workgroup of DEC_WAVES waves owns one contiguous chunk of a (batch, head)'s tiles, and the S axis is cut into
// dec_nsplit chunks so that about DEC_WG_PER_CU workgroups per compute unit exist however small B * H is.  A chunk holds at least
// DEC_MIN_TILES tiles (one per wave) unless S itself is shorter, at most DEC_MAX_SPLIT chunks exist, and none is empty: the count is
// re-derived from the chunk's length.  cus <= 0: the MI355X's 256.
constexpr int DEC_TILE = 32;
constexpr int DEC_WAVES = 4;
constexpr int DEC_MIN_TILES = 4;
constexpr int DEC_MAX_SPLIT = 64;
constexpr int DEC_WG_PER_CU = 2;
constexpr int DEC_MAX_T = 16;
inline int64_t dec_tiles(int64_t S) { return (S + DEC_TILE - 1) / DEC_TILE; }
// tiles of one chunk
inline int64_t dec_chunk_tiles(int64_t bh, int64_t S, int64_t cus) {
    const int64_t nt = dec_tiles(S), wgs = (cus > 0 ? cus : 256) * DEC_WG_PER_CU;
    int64_t n = (wgs + bh - 1) / bh;                                        // chunks wanted
    const int64_t most = nt / DEC_MIN_TILES > 1 ? nt / DEC_MIN_TILES : 1;   // chunks S can fill
    n = n < most ? n : most;
    n = n < DEC_MAX_SPLIT ? n : DEC_MAX_SPLIT;
    return (nt + n - 1) / n;
}
inline int64_t dec_nsplit(int64_t bh, int64_t S, int64_t cus) {
    const int64_t per = dec_chunk_tiles(bh, S, cus);
    return (dec_tiles(S) + per - 1) / per;
}

// Work split of the prefill attention (fq_attn_prefill.h): grid (pre_query_tiles(T), B * H).  A workgroup of PRE_WAVES waves owns PRE_QT
// query rows, PRE_RPW of them per wave (a multiple of 16: the B operands that share every K and V fragment), and walks all S keys in
// tiles of PRE_KT; there is no split along S.  PRE_RPW is an A/B macro (DESIGN.md section 31 has 16 against 32).
#ifndef PRE_RPW
#define PRE_RPW 32
#endif
constexpr int PRE_WAVES = 4;
constexpr int PRE_KT = 32;
constexpr int PRE_QT = PRE_WAVES * PRE_RPW;
constexpr int64_t PRE_MAX_GRID_Y = 65535;
static_assert(PRE_RPW == 16 || PRE_RPW == 32, "one or two 16-row blocks a wave");
inline int64_t pre_query_tiles(int64_t T) { return (T + PRE_QT - 1) / PRE_QT; }

// Work split of the training attention's backward (fq_attn_train.h): two launches.  The dq kernel has the forward's split: grid
// (trn_query_tiles(T), B * H), a workgroup of TRN_WAVES waves owns TRN_DQ_QT query rows, TRN_RPW of them per wave, and walks the keys
// in tiles of TRN_DQ_KT.  The dk/dv kernel is its mirror: grid (trn_key_tiles(S), B * H), a workgroup owns TRN_DKV_KT keys, TRN_KPW of
// them per wave, and walks the query rows in tiles of TRN_DKV_QT.  TRN_RPW and TRN_KPW are A/B macros.
#ifndef TRN_RPW
#define TRN_RPW 32
#endif
#ifndef TRN_KPW
#define TRN_KPW 16
#endif
constexpr int TRN_WAVES = 4;
constexpr int TRN_DQ_QT = TRN_WAVES * TRN_RPW;
constexpr int TRN_DQ_KT = 32;
constexpr int TRN_DKV_KT = TRN_WAVES * TRN_KPW;
constexpr int TRN_DKV_QT = 32;
static_assert((TRN_RPW == 16 || TRN_RPW == 32) && (TRN_KPW == 16 || TRN_KPW == 32), "one or two 16-row / 16-key blocks a wave");
inline int64_t trn_query_tiles(int64_t T) { return (T + TRN_DQ_QT - 1) / TRN_DQ_QT; }
inline int64_t trn_key_tiles(int64_t S) { return (S + TRN_DKV_KT - 1) / TRN_DKV_KT; }

}  // namespace fq
