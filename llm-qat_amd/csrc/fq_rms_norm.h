// fq_rms_norm.h -- the root-mean-square layer norm  y = w * (x * rsqrt(mean(x^2) + eps))  and its gradients: the
// kernels behind include/llmqat_fakequant_norm.h.  fp32 arithmetic whatever the dtypes, in the reference's op order with its roundings
// (models/modeling_llama_quant.py:112-129); no fp32 [rows, cols] tensor ever exists.  It stands on the row layer of fq_rows.h: the
// launch shape, unpack / pack, the one-barrier reduction over a row's waves.
//
//   rms_fwd_kernel   one row per workgroup (rows of ROW_WIDE elements or more) or per wave.  A lane reads one SWEEP of the row into
//                    registers (RmsIO: NS slots), sums the squares in slot order, the lanes' sums are added (DPP butterfly, then the waves
//                    through LDS in wave order: a fixed order), rstd = v_rsq_f32(ss / cols + eps), and the sweep is scaled from the
//                    registers: a row of up to SWEEP elements (8192 on the 16-byte path of a workgroup, 4096 on the element path) is read
//                    once.  Wider rows sum over further sweeps and read themselves again for the scaling.  The 16-byte kernels are
//                    built for a quarter, a half and all of RMS_VIF vectors per lane, and a row takes the smallest that holds it.
//   rms_bwd_kernel   part p (a workgroup, or a wave for short rows) owns rows [p * rpp, (p + 1) * rpp).  Per row: a = g w, n = x rstd,
//                    s = sum(a n) / cols (one reduction), dx = rstd (a - n s); g n is accumulated per column in registers across the
//                    part's rows, in row order, and written once as the part's fp32 row of the workspace.  Rows wider than a sweep
//                    accumulate in the part's workspace row itself (private to the part: read, add, write by the same lane).
//   rms_dw_kernel    dw[c] = the parts' partial sums of column c: RMS_DW_SEGS runs of consecutive parts, each summed in index order by one
//                    thread, then the runs in index order.  No atomics: the order is a function of the shape alone.
//
// RmsIO maps a lane's slots to columns.  16-byte path (equal dtypes, every base pointer 16-byte aligned, a row whole vectors): group i is
// vector i * TPR + lane of the sweep, EPV elements.  Element path (any cols, any alignment, the mixed-dtype pairs): group i is the element
// i * TPR + lane.  The arithmetic sees slots only, so both paths compute the same values.  A slot past the end of the row holds 0, which
// adds nothing to any of the sums, and is never stored.
//
// Special values follow the chain: a NaN makes its row's sums, hence the row's y and dx and every dw it reaches, NaN, and no other row's;
// +-inf gives ss = inf, rstd = 0, NaN at the inf and 0 elsewhere; a sum of squares that overflows likewise gives rstd = 0 and zeros.
// RMS_NT_LOAD / RMS_NT_STORE / RMS_VIF: cache policies of the 16-byte streams and 16-byte vectors of a 16-bit tensor a lane holds per sweep
// (an fp32 tensor: twice as many), A/B macros as CE_* are.
#pragma once
#include "fq_rows.h"

#ifndef RMS_NT_LOAD
#define RMS_NT_LOAD 0     // x was written by the kernel just before, and the backward reads it again
#endif
#ifndef RMS_NT_STORE
#define RMS_NT_STORE 1    // as the losses' gradients: a plain store leaves the lines dirty in the caches
#endif
#ifndef RMS_VIF
#define RMS_VIF 4         // 4 * 8 * 256 = 8192 elements of a workgroup's row in registers
#endif
#ifndef RMS_BWD_PARTS_WIDE
#define RMS_BWD_PARTS_WIDE 512      // workgroups of the backward at most (rows of ROW_WIDE elements or more)
#endif
#ifndef RMS_BWD_PARTS_NARROW
#define RMS_BWD_PARTS_NARROW 2048   // waves of the backward at most (shorter rows)
#endif

namespace fq {

// elements of a lane per sweep on the element path: a sweep of 4096 columns for a workgroup, 1024 for a wave.  Half the 16-byte path's 32
// slots: the backward holds x, g, w and the sums per slot and sits at 215 VGPRs with 16.  So on this path (mixed dtypes, an unaligned base,
// a row that is not whole vectors) the forward reads a row of 4097 .. 8192 elements twice; the second read follows the first within the
// same workgroup, on at most 32 KB
constexpr int RMS_EG = 16;
constexpr int RMS_DW_COLS = 16, RMS_DW_SEGS = 16;   // rms_dw_kernel: columns of a workgroup, runs of parts per column
constexpr int RMS_DW_TPB = RMS_DW_COLS * RMS_DW_SEGS;

struct RmsFwdArgs {
    const void* x;
    const void* w;
    void* y;
    float* rstd;      // [rows] or nullptr
    int64_t rows, cols;
    float eps;
};
struct RmsBwdArgs {
    const void* g;
    const void* x;
    const void* w;
    const float* rstd;
    void* dx;         // or nullptr: not stored
    float* ws;        // [parts, cols] or nullptr: no partial sums
    int64_t rows, cols, parts, rpp;
};

// the most 16-byte vectors of a lane per sweep, and the three counts a kernel is built for: a row of 4096 bf16 elements needs two of a
// workgroup's lanes, and a kernel built for four would carry twice the registers (half the waves per SIMD) and load the rest for nothing
template <int DT> constexpr int rms_most_groups() { return RMS_VIF * Ty<DT>::ESIZE / 2; }
constexpr int rms_groups(int most, int step) { return (most >> step) > 0 ? most >> step : 1; }      // step 0, 1, 2: most, a half, a quarter

template <int DT, bool VEC, int TPR, int NGV> struct RmsIO {
    using T = Ty<DT>;
    static constexpr int EPV = VEC ? 16 / T::ESIZE : 1;                   // elements of a group
    static constexpr int NG = VEC ? NGV : RMS_EG;                         // groups of a lane per sweep (NGV: the 16-byte path's)
    static constexpr int NS = NG * EPV;                                   // slots of a lane per sweep
    static constexpr int64_t SWEEP = (int64_t)NS * TPR;                   // columns of a sweep

    // the sweep that starts at column c0 (< cols) of the row that starts at element `base` of p; slots past the row are 0, and their
    // address the sweep's first group
    template <bool NT> __device__ static __forceinline__ void load(const void* p, int64_t base, int64_t c0, int64_t cols, int lane, float (&f)[NS]) {
        if constexpr (VEC) {
            const uint4* pv = (const uint4*)((const char*)p + (base + c0) * T::ESIZE);
            const int64_t nvec = (cols - c0) / EPV;
            uint4 r[NG];
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const int64_t vi = (int64_t)i * TPR + lane;
                r[i] = ld16<NT>(pv + (vi < nvec ? vi : 0));
            }
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                float e[EPV];
                row_unpack<DT>(r[i], e);
                const bool in = (int64_t)i * TPR + lane < nvec;
#pragma unroll
                for (int k = 0; k < EPV; ++k) f[i * EPV + k] = in ? e[k] : 0.0f;
            }
        } else {
            // (not row_load_group: a lane's first column, which that clamps to, may lie past the row here, where every lane of the row
            // loads; with a clamp that tests for it the element-path kernels differ, v_cndmask_b32 220 -> 252 in the backwards)
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const int64_t c = c0 + (int64_t)i * TPR + lane;
                const bool in = c < cols;
                const float v = T::load1(p, base + (in ? c : c0));
                f[i] = in ? v : 0.0f;
            }
        }
    }
    // the same slots back, rounded once to DT; slots past the row are not stored
    template <bool NT> __device__ static __forceinline__ void store(void* p, int64_t base, int64_t c0, int64_t cols, int lane, const float (&f)[NS]) {
        if constexpr (VEC) {
            uint4* pv = (uint4*)((char*)p + (base + c0) * T::ESIZE);
            const int64_t nvec = (cols - c0) / EPV;
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const int64_t vi = (int64_t)i * TPR + lane;
                float e[EPV];
#pragma unroll
                for (int k = 0; k < EPV; ++k) e[k] = f[i * EPV + k];
                if (vi < nvec) st16<NT>(pv + vi, row_pack<DT>(e));
            }
        } else {
#pragma unroll
            for (int i = 0; i < NG; ++i) {
                const int64_t c = c0 + (int64_t)i * TPR + lane;
                if (c < cols) T::store1(p, base + c, f[i]);
            }
        }
    }
    // the slots as fp32 at their columns of a workspace row (which starts at element `base` of ws): read (0 past the row) and write
    __device__ static __forceinline__ void load_f32(const float* ws, int64_t base, int64_t c0, int64_t cols, int lane, float (&f)[NS]) {
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int64_t c = c0 + ((int64_t)i * TPR + lane) * EPV;
            const bool in = c < cols;      // a group is inside the row or outside it as a whole
            if constexpr (VEC) {
#pragma unroll
                for (int q = 0; q < EPV / 4; ++q) {
                    const uint4 v = *(const uint4*)(ws + base + (in ? c : c0) + 4 * q);
                    f[i * EPV + 4 * q + 0] = in ? as_f(v.x) : 0.0f;
                    f[i * EPV + 4 * q + 1] = in ? as_f(v.y) : 0.0f;
                    f[i * EPV + 4 * q + 2] = in ? as_f(v.z) : 0.0f;
                    f[i * EPV + 4 * q + 3] = in ? as_f(v.w) : 0.0f;
                }
            } else {
                const float v = ws[base + (in ? c : c0)];
                f[i] = in ? v : 0.0f;
            }
        }
    }
    __device__ static __forceinline__ void store_f32(float* ws, int64_t base, int64_t c0, int64_t cols, int lane, const float (&f)[NS]) {
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int64_t c = c0 + ((int64_t)i * TPR + lane) * EPV;
            if (c < cols) {
                if constexpr (VEC) {
#pragma unroll
                    for (int q = 0; q < EPV / 4; ++q)
                        *(uint4*)(ws + base + c + 4 * q) = make_uint4(as_u(f[i * EPV + 4 * q]), as_u(f[i * EPV + 4 * q + 1]),
                                                                       as_u(f[i * EPV + 4 * q + 2]), as_u(f[i * EPV + 4 * q + 3]));
                } else {
                    ws[base + c] = f[i];
                }
            }
        }
    }
};

// y's slots from x's and w's: n = x rstd rounded once to fp32; a 16-bit w rounds n to its dtype first (the store rounds the product)
template <int WDT, int N> __device__ __forceinline__ void rms_scale(float (&x)[N], const float (&w)[N], float rstd) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float n = x[i] * rstd;
        // fp16: left to itself the compiler makes the multiply and the conversion one v_fma_mixlo_f16, which rounds the exact product once
        // to fp16; the chain rounds to fp32 first, and an fp32 product that is a tie between two fp16 values then goes the other way
        if constexpr (WDT == F16) asm("" : "+v"(n));
        float y = w[i] * Ty<WDT>::rb(n);
        // and the product with w, fused with its conversion, becomes v_fma_mixlo_f16(w, n, +0): -0 + +0 = +0 loses the sign of a zero
        if constexpr (WDT == F16) asm("" : "+v"(y));
        x[i] = y;
    }
}

template <int XDT, int WDT, bool VEC, int TPR, int NGV>
__global__ __launch_bounds__(ROW_TPB) void rms_fwd_kernel(RmsFwdArgs a) {
    using IX = RmsIO<XDT, VEC, TPR, NGV>;
    using IW = RmsIO<WDT, VEC, TPR, NGV>;
    constexpr int NS = IX::NS, NW = TPR / 64;
    static_assert(IX::NS == IW::NS, "x and w share the slots");
    __shared__ uint32_t lds[1][4];
    int64_t row;
    int lane;
    if (!row_lane<TPR>(a.rows, row, lane)) return;
    const int64_t base = row * a.cols;
    float f[NS];
    IX::template load<RMS_NT_LOAD != 0>(a.x, base, 0, a.cols, lane, f);
    float ss = 0.0f;
#pragma unroll
    for (int i = 0; i < NS; ++i) ss += f[i] * f[i];
    for (int64_t c0 = IX::SWEEP; c0 < a.cols; c0 += IX::SWEEP) {
        float t[NS];
        IX::template load<RMS_NT_LOAD != 0>(a.x, base, c0, a.cols, lane, t);
#pragma unroll
        for (int i = 0; i < NS; ++i) ss += t[i] * t[i];
    }
    uint32_t v[1] = {as_u(ss)};
    row_reduce<OpAddF, NW>(v, lds);
    const float rstd = __builtin_amdgcn_rsqf(as_f(v[0]) / (float)a.cols + a.eps);
    if (lane == 0 && a.rstd) a.rstd[row] = rstd;
    // (load w, scale, store: written out twice.  As one helper 15 kernels are reordered and 5 differ, the bf16 16-byte forwards of one
    // vector by 37 -> 41 VGPRs)
    if (a.cols <= IX::SWEEP) {              // the row is in registers
        float w[NS];
        IW::template load<false>(a.w, 0, 0, a.cols, lane, w);
        rms_scale<WDT>(f, w, rstd);
        IW::template store<RMS_NT_STORE != 0>(a.y, base, 0, a.cols, lane, f);
    } else {
        for (int64_t c0 = 0; c0 < a.cols; c0 += IX::SWEEP) {
            float w[NS];
            IX::template load<RMS_NT_LOAD != 0>(a.x, base, c0, a.cols, lane, f);
            IW::template load<false>(a.w, 0, c0, a.cols, lane, w);
            rms_scale<WDT>(f, w, rstd);
            IW::template store<RMS_NT_STORE != 0>(a.y, base, c0, a.cols, lane, f);
        }
    }
}

// the sweep that starts at column c0 of one row of the backward: x and g are loaded, and w with LOADW (else it is the caller's, loaded once
// for all rows); x -> n = x rstd, g -> a = g w, gn = g n (n is not rounded); -> the lane's part of sum(a n).  (The tensors come as pointers:
// with the RmsBwdArgs by reference four element-path kernels lose a v_mov_b32 and ten more are reordered.  As it stands the 18 kernels
// of the 16-byte path are reordered, two base addresses trading registers, and the rest identical: DESIGN.md section 26)
template <class IX, class IW, bool LOADW, int N>
__device__ __forceinline__ float rms_bwd_sweep(const void* pg, const void* px, const void* pw, int64_t cols, int64_t base, int64_t c0, int lane,
                                               float rstd, float (&x)[N], float (&g)[N], float (&gn)[N], float (&w)[N]) {
    IX::template load<RMS_NT_LOAD != 0>(px, base, c0, cols, lane, x);
    IW::template load<RMS_NT_LOAD != 0>(pg, base, c0, cols, lane, g);
    if constexpr (LOADW) IW::template load<false>(pw, 0, c0, cols, lane, w);
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x[i] = x[i] * rstd;
        gn[i] = g[i] * x[i];
        g[i] = g[i] * w[i];
        p += g[i] * x[i];
    }
    return p;
}
// dx's slots into a: rstd (a - n s)
template <int XDT, int N> __device__ __forceinline__ void rms_dx(float (&a)[N], const float (&n)[N], float s, float rstd) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float d = rstd * (a[i] - n[i] * s);
        if constexpr (XDT == F16) asm("" : "+v"(d));      // as rms_scale: the fp32 product, then one conversion
        a[i] = d;
    }
}

template <int XDT, int WDT, bool VEC, int TPR, int NGV>
__global__ __launch_bounds__(ROW_TPB) void rms_bwd_kernel(RmsBwdArgs a) {
    using IX = RmsIO<XDT, VEC, TPR, NGV>;
    using IW = RmsIO<WDT, VEC, TPR, NGV>;
    constexpr int NS = IX::NS, NW = TPR / 64;
    static_assert(IX::NS == IW::NS, "x, g and w share the slots");
    __shared__ uint32_t lds[2][1][4];       // two, used in turn: a row's sums are read while the next row's are written
    int64_t part;
    int lane;
    if (!row_lane<TPR>(a.parts, part, lane)) return;
    const int64_t r0 = part * a.rpp, r1 = r0 + a.rpp < a.rows ? r0 + a.rpp : a.rows;
    const int64_t wsb = part * a.cols;
    int par = 0;
    if (a.cols <= IX::SWEEP) {              // a row is in registers, and so are the part's sums of g n
        float w[NS], acc[NS];
        IW::template load<false>(a.w, 0, 0, a.cols, lane, w);
#pragma unroll
        for (int i = 0; i < NS; ++i) acc[i] = 0.0f;
        for (int64_t row = r0; row < r1; ++row, par ^= 1) {
            const int64_t base = row * a.cols;
            const float rstd = a.rstd[row];
            float x[NS], g[NS], gn[NS];
            uint32_t v[1] = {as_u(rms_bwd_sweep<IX, IW, false>(a.g, a.x, a.w, a.cols, base, 0, lane, rstd, x, g, gn, w))};
            row_reduce<OpAddF, NW>(v, lds[par]);
            if (a.ws) {
#pragma unroll
                for (int i = 0; i < NS; ++i) acc[i] += gn[i];
            }
            if (a.dx) {
                rms_dx<XDT>(g, x, as_f(v[0]) / (float)a.cols, rstd);
                IX::template store<RMS_NT_STORE != 0>(a.dx, base, 0, a.cols, lane, g);
            }
        }
        if (a.ws) IX::store_f32(a.ws, wsb, 0, a.cols, lane, acc);
    } else {
        for (int64_t row = r0; row < r1; ++row, par ^= 1) {
            const int64_t base = row * a.cols;
            const float rstd = a.rstd[row];
            float p = 0.0f;
            for (int64_t c0 = 0; c0 < a.cols; c0 += IX::SWEEP) {
                float x[NS], g[NS], gn[NS], w[NS];
                p += rms_bwd_sweep<IX, IW, true>(a.g, a.x, a.w, a.cols, base, c0, lane, rstd, x, g, gn, w);
            }
            uint32_t v[1] = {as_u(p)};
            row_reduce<OpAddF, NW>(v, lds[par]);
            const float s = as_f(v[0]) / (float)a.cols;
            for (int64_t c0 = 0; c0 < a.cols; c0 += IX::SWEEP) {
                float x[NS], g[NS], gn[NS], w[NS];
                rms_bwd_sweep<IX, IW, true>(a.g, a.x, a.w, a.cols, base, c0, lane, rstd, x, g, gn, w);
                if (a.ws) {
                    if (row > r0) {         // the part's own row of the workspace: the lane that wrote a column is the one that reads it
                        float acc[NS];
                        IX::load_f32(a.ws, wsb, c0, a.cols, lane, acc);
#pragma unroll
                        for (int i = 0; i < NS; ++i) gn[i] = acc[i] + gn[i];
                    }
                    IX::store_f32(a.ws, wsb, c0, a.cols, lane, gn);
                }
                if (a.dx) {
                    rms_dx<XDT>(g, x, s, rstd);
                    IX::template store<RMS_NT_STORE != 0>(a.dx, base, c0, a.cols, lane, g);
                }
            }
        }
    }
}

template <int WDT>
__global__ __launch_bounds__(RMS_DW_TPB) void rms_dw_kernel(const float* ws, void* dw, int64_t parts, int64_t cols) {
    __shared__ float sh[RMS_DW_SEGS][RMS_DW_COLS];
    const int ci = threadIdx.x % RMS_DW_COLS, seg = threadIdx.x / RMS_DW_COLS;
    const int64_t c = (int64_t)blockIdx.x * RMS_DW_COLS + ci;
    const int64_t per = (parts + RMS_DW_SEGS - 1) / RMS_DW_SEGS;
    const int64_t p0 = seg * per, p1 = p0 + per < parts ? p0 + per : parts;
    float acc = 0.0f;
    if (c < cols) {
#pragma unroll 8
        for (int64_t p = p0; p < p1; ++p) acc += ws[p * cols + c];
    }
    sh[seg][ci] = acc;
    __syncthreads();
    if (seg == 0 && c < cols) {
        float r = sh[0][ci];
#pragma unroll
        for (int s = 1; s < RMS_DW_SEGS; ++s) r += sh[s][ci];
        Ty<WDT>::store1(dw, c, r);
    }
}

// ---- host part: the chunks of the backward, a function of the shape alone ---------------------------------------------------------------
inline int64_t rms_rows_per_part(int64_t rows, int64_t cols) {
    const int64_t most = row_wide(cols) ? RMS_BWD_PARTS_WIDE : RMS_BWD_PARTS_NARROW;
    return (rows + most - 1) / most;
}
inline int64_t rms_parts(int64_t rows, int64_t cols) {
    const int64_t rpp = rms_rows_per_part(rows, cols);
    return (rows + rpp - 1) / rpp;          // every part has a row, and rpp == ceil(rows / parts)
}

}  // namespace fq
