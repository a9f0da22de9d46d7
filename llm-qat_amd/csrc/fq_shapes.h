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

}  // namespace fq
