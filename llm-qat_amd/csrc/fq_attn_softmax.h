// fq_attn_softmax.h -- the chain between the two attention products: the kernels behind
// include/llmqat_fakequant_attn.h.
//
//   attn = scores / sqrt(head_dim);  attn = attn + mask;  attn = max(attn, finfo.min);  y = softmax(attn, -1, float32).to(dtype)
//
// as one forward and one backward kernel over rows of scores, in fp32 arithmetic with the chain's roundings in front of the softmax.  No
// fp32 [B, H, T, S] tensor ever exists; the backward needs the scores, the mask and two floats per row.  It stands on the row layer of
// fq_rows.h (launch shape, unpack / pack, the one-barrier reduction) and the softmax layer of fq_loss_rows.h (exponentials, reference point).
//
//   attn_fwd_kernel   one row per workgroup (rows of ROW_WIDE elements or more) or per wave.  A lane reads one SWEEP of the row and of the
//                     mask row into registers, z = clamp(rb_P(rb(x inv) + m)) per slot, the maximum over the row (v_max_f32, DPP butterfly,
//                     then the waves through LDS), e = exp(z - max) summed in slot order, the lanes' sums added in a fixed order,
//                     y = rb(e (1 / sum)), stored from the registers: a row of up to SWEEP elements is read once.  Wider rows make three
//                     passes over themselves (maximum, sum, store).  stats[row] = (max, sum).
//   attn_bwd_kernel   the same slots: p = exp(z - max) (1 / sum) from the stored stats with the forward's own device functions (attn_z,
//                     attn_p), so p is the forward's fp32 p bit for bit; dot = sum(g p) in slot order, then the fixed reduction;
//                     d = (g - dot) p, rounded to P, the gradient of max (1, 1/2 at a tie, 0 below), rounded to the dtype, times inv.
//                     Rows wider than a sweep make two passes.
//
// Slots.  AttnGeom maps a lane's slots to columns.  16-byte path: group i is the EPV consecutive columns (i * TPR + lane) * EPV of the
// sweep, one 16-byte vector of the scores; the mask's group is the same columns, one vector where it has the scores' dtype and two
// consecutive ones where it is fp32 beside 16-bit scores (the pair autocast over fp32 weights runs), so the mixed pairs take this path
// too.  Element path (any cols, any alignment): group i is the column i * TPR + lane.  The arithmetic sees slots only.  A slot past the
// end of the row is -inf BEHIND the clamp (clamped it would count in a fully masked row's sum) and is never stored.
//
// The mask row of (batch b, token t) is read by the H heads of b: plain loads, so the heads after the first find it in the caches.
//
// Special values.  A NaN element makes its row's sum, hence the row, NaN (v_max_f32 ignores it, e^(NaN - m) does not); +inf gives
// inf - inf = NaN likewise.  -inf under a mask becomes MIN_P; without a mask a row of only -inf has reference point 0 (loss_ref), sum 0,
// and is NaN as ATen's.  MIN_P - max overflows to -inf or is about -3.4e38: both exponentials give 0 there.
//
// ATTN_NT_LOAD / ATTN_NT_STORE / ATTN_VIF / ATTN_EXP_ACC: cache policies of the 16-byte streams, 16-byte vectors of a 16-bit tensor a lane
// holds per sweep (fp32: twice as many), and which exponential of fq_loss_rows.h: A/B macros, as RMS_* are.
#pragma once
#include "fq_loss_rows.h"

#ifndef ATTN_NT_LOAD
#define ATTN_NT_LOAD 0     // the scores were written by the product just before, and the backward reads them again
#endif
#ifndef ATTN_NT_STORE
#define ATTN_NT_STORE 1    // as the norm's and the losses' results
#endif
#ifndef ATTN_VIF
#define ATTN_VIF 4         // 4 * 8 * 256 = 8192 columns of a workgroup's row in registers, 2048 of a wave's
#endif
#ifndef ATTN_EXP_ACC
#define ATTN_EXP_ACC 0     // loss_exp, the cheaper one: the caps hold with it (DESIGN.md section 29 has both exponentials' measures)
#endif

namespace fq {

constexpr int ATTN_EG = 16;          // elements of a lane per sweep on the element path: 4096 columns for a workgroup, 1024 for a wave
constexpr int ATTN_NOMASK = -1;      // the mask's dtype parameter where there is none

struct AttnMask {
    const void* p;       // [B, 1, T, S] by strides, last stride 1
    int64_t bs, rs;      // batch and row stride in elements
    int64_t ht, t;       // H * T and T: row = (b * H + h) * T + t
};
struct AttnFwdArgs {
    const void* x;
    AttnMask m;
    void* y;
    float* stats;        // [rows, 2] or nullptr
    int64_t rows, cols;
    float inv;
};
struct AttnBwdArgs {
    const void* g;
    const void* x;
    AttnMask m;
    const float* stats;
    void* dx;
    int64_t rows, cols;
    float inv;
};

// the dtype of scores + mask, and its most negative finite value
template <int DT, int MDT> constexpr int attn_sum_dtype() { return MDT == ATTN_NOMASK || MDT == DT ? DT : F32; }
template <int P> __device__ __forceinline__ float attn_min() { return as_f(P == F32 ? 0xFF7FFFFFu : P == BF16 ? 0xFF7F0000u : 0xC77FE000u); }

__device__ __forceinline__ float attn_exp(float d) {
#if ATTN_EXP_ACC
    return loss_exp_acc(d);
#else
    return loss_exp(d);
#endif
}

template <int DT, bool VEC_, int TPR_, int NGV> struct AttnGeom {
    static constexpr bool VEC = VEC_;
    static constexpr int TPR = TPR_;
    static constexpr int EPV = VEC ? 16 / Ty<DT>::ESIZE : 1;             // columns of a group
    static constexpr int NG = VEC ? NGV : ATTN_EG;                       // groups of a lane per sweep
    static constexpr int NS = NG * EPV;                                  // slots of a lane per sweep
    static constexpr int64_t SWEEP = (int64_t)NS * TPR;                  // columns of a sweep
    // is group i of the sweep that starts at column c0 inside the row (on the 16-byte path a row is whole groups)
    __device__ static __forceinline__ bool in(int i, int64_t c0, int64_t cols, int lane) { return c0 + ((int64_t)i * TPR + lane) * EPV < cols; }
};

// the sweep that starts at column c0 (< cols) of the row that starts at element `base` of p, a tensor of dtype EDT, as floats.  Slots
// past the row hold the sweep's first group (an address inside the row) and are the caller's to replace
template <int EDT, bool NT, class G> __device__ __forceinline__ void attn_load(const void* p, int64_t base, int64_t c0, int64_t cols, int lane, float (&f)[G::NS]) {
    using T = Ty<EDT>;
    if constexpr (G::VEC) {
        constexpr int NV = G::EPV * T::ESIZE / 16;      // 16-byte vectors of a group: 1, or 2 for an fp32 mask beside 16-bit scores
        constexpr int EPL = 16 / T::ESIZE;              // elements of a vector
        static_assert(NV >= 1 && NV * EPL == G::EPV, "a group is whole vectors");
        const uint4* pv = (const uint4*)((const char*)p + (base + c0) * T::ESIZE);
        const int64_t ngrp = (cols - c0) / G::EPV;
        uint4 r[G::NG][NV];
#pragma unroll
        for (int i = 0; i < G::NG; ++i) {
            const int64_t gi = (int64_t)i * G::TPR + lane;
            const int64_t at = (gi < ngrp ? gi : 0) * NV;
#pragma unroll
            for (int k = 0; k < NV; ++k) r[i][k] = ld16<NT>(pv + at + k);
        }
#pragma unroll
        for (int i = 0; i < G::NG; ++i) {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                float e[EPL];
                row_unpack<EDT>(r[i][k], e);
#pragma unroll
                for (int j = 0; j < EPL; ++j) f[i * G::EPV + k * EPL + j] = e[j];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < G::NG; ++i) {
            const int64_t c = c0 + (int64_t)i * G::TPR + lane;
            f[i] = T::load1(p, base + (c < cols ? c : c0));
        }
    }
}
// the same slots back, rounded once to DT; slots past the row are not stored
template <int DT, bool NT, class G> __device__ __forceinline__ void attn_store(void* p, int64_t base, int64_t c0, int64_t cols, int lane, const float (&f)[G::NS]) {
    using T = Ty<DT>;
    if constexpr (G::VEC) {
        uint4* pv = (uint4*)((char*)p + (base + c0) * T::ESIZE);
        const int64_t ngrp = (cols - c0) / G::EPV;
#pragma unroll
        for (int i = 0; i < G::NG; ++i) {
            const int64_t gi = (int64_t)i * G::TPR + lane;
            float e[G::EPV];
#pragma unroll
            for (int k = 0; k < G::EPV; ++k) e[k] = f[i * G::EPV + k];
            if (gi < ngrp) st16<NT>(pv + gi, row_pack<DT>(e));
        }
    } else {
#pragma unroll
        for (int i = 0; i < G::NG; ++i) {
            const int64_t c = c0 + (int64_t)i * G::TPR + lane;
            if (c < cols) T::store1(p, base + c, f[i]);
        }
    }
}

// where the mask row of `row` starts, in elements
template <int MDT> __device__ __forceinline__ int64_t attn_mask_base(const AttnMask& m, int64_t row, int64_t rows) {
    if constexpr (MDT == ATTN_NOMASK) {
        return 0;
    } else {
        int64_t b, t;
        if ((rows >> 32) == 0) {            // H * T and T divide the rows: where those fit 32 bits, so does this arithmetic
            b = (uint32_t)row / (uint32_t)m.ht;
            t = (uint32_t)row % (uint32_t)m.t;
        } else {
            b = row / m.ht;
            t = row % m.t;
        }
        return b * m.bs + t * m.rs;
    }
}

// a = rb_P(rb(x inv) + m), the chain's value in front of the clamp; without a mask rb(x inv)
template <int DT, int MDT> __device__ __forceinline__ float attn_a(float x, float m, float inv) {
    constexpr int P = attn_sum_dtype<DT, MDT>();
    float t = x * inv;
    // fp16: left to itself the compiler makes a product or a sum and its conversion one v_fma_mixlo_f16, which rounds once; the chain
    // rounds to fp32 first (fq_rms_norm.h rms_scale)
    if constexpr (DT == F16) asm("" : "+v"(t));
    t = Ty<DT>::rb(t);
    if constexpr (MDT == ATTN_NOMASK) {
        return t;
    } else {
        float a = t + m;
        if constexpr (P == F16) asm("" : "+v"(a));
        return Ty<P>::rb(a);
    }
}
// z = max(a, MIN_P): -inf becomes MIN_P, NaN stays; no clamp without a mask (the reference clamps under a mask only)
template <int DT, int MDT> __device__ __forceinline__ float attn_z(float a) {
    if constexpr (MDT == ATTN_NOMASK) {
        return a;
    } else {
        const float mn = attn_min<attn_sum_dtype<DT, MDT>()>();
        return a < mn ? mn : a;
    }
}
// p from z and the row's stats: the one formulation of both kernels
__device__ __forceinline__ float attn_p(float z, float ref, float rinv) { return attn_exp(z - ref) * rinv; }

// one sweep's a (the chain's values in front of the clamp; slots past the row hold a real element's)
template <int DT, int MDT, class G>
__device__ __forceinline__ void attn_a_sweep(const void* px, const void* pm, int64_t base, int64_t mbase, int64_t c0, int64_t cols, int lane,
                                             float inv, float (&a)[G::NS]) {
    attn_load<DT, ATTN_NT_LOAD != 0, G>(px, base, c0, cols, lane, a);
    if constexpr (MDT == ATTN_NOMASK) {
#pragma unroll
        for (int i = 0; i < G::NS; ++i) a[i] = attn_a<DT, MDT>(a[i], 0.0f, inv);
    } else {
        float m[G::NS];
        attn_load<MDT, false, G>(pm, mbase, c0, cols, lane, m);
#pragma unroll
        for (int i = 0; i < G::NS; ++i) a[i] = attn_a<DT, MDT>(a[i], m[i], inv);
    }
}
// a -> z in place, slots past the row -inf
template <int DT, int MDT, class G> __device__ __forceinline__ void attn_z_slots(float (&a)[G::NS], int64_t c0, int64_t cols, int lane) {
#pragma unroll
    for (int i = 0; i < G::NG; ++i) {
        const bool in = G::in(i, c0, cols, lane);
#pragma unroll
        for (int k = 0; k < G::EPV; ++k) a[i * G::EPV + k] = in ? attn_z<DT, MDT>(a[i * G::EPV + k]) : LOSS_NEG_INF;
    }
}

template <int DT, int MDT, bool VEC, int TPR, int NGV>
__global__ __launch_bounds__(ROW_TPB) void attn_fwd_kernel(AttnFwdArgs a) {
    using G = AttnGeom<DT, VEC, TPR, NGV>;
    constexpr int NS = G::NS, NW = TPR / 64;
    __shared__ uint32_t lds_max[1][4], lds_sum[1][4];
    int64_t row;
    int lane;
    if (!row_lane<TPR>(a.rows, row, lane)) return;
    const int64_t base = row * a.cols;
    const int64_t mbase = attn_mask_base<MDT>(a.m, row, a.rows);
    const bool one = a.cols <= G::SWEEP;        // the row is in registers
    float z[NS];
    attn_a_sweep<DT, MDT, G>(a.x, a.m.p, base, mbase, 0, a.cols, lane, a.inv, z);
    attn_z_slots<DT, MDT, G>(z, 0, a.cols, lane);
    float mx = z[0];
#pragma unroll
    for (int i = 1; i < NS; ++i) mx = __builtin_fmaxf(mx, z[i]);
    for (int64_t c0 = G::SWEEP; c0 < a.cols; c0 += G::SWEEP) {
        float t[NS];
        attn_a_sweep<DT, MDT, G>(a.x, a.m.p, base, mbase, c0, a.cols, lane, a.inv, t);
        attn_z_slots<DT, MDT, G>(t, c0, a.cols, lane);
#pragma unroll
        for (int i = 0; i < NS; ++i) mx = __builtin_fmaxf(mx, t[i]);
    }
    uint32_t vm[1] = {as_u(mx)};
    row_reduce<OpMaxF, NW>(vm, lds_max);
    mx = as_f(vm[0]);
    const float ref = loss_ref(mx);
    float s = 0.0f;
    if (one) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            z[i] = attn_exp(z[i] - ref);
            s += z[i];
        }
    } else {
        for (int64_t c0 = 0; c0 < a.cols; c0 += G::SWEEP) {
            float t[NS];
            attn_a_sweep<DT, MDT, G>(a.x, a.m.p, base, mbase, c0, a.cols, lane, a.inv, t);
            attn_z_slots<DT, MDT, G>(t, c0, a.cols, lane);
#pragma unroll
            for (int i = 0; i < NS; ++i) s += attn_exp(t[i] - ref);
        }
    }
    uint32_t vs[1] = {as_u(s)};
    row_reduce<OpAddF, NW>(vs, lds_sum);
    s = as_f(vs[0]);
    if (lane == 0 && a.stats) {
        a.stats[2 * row] = mx;
        a.stats[2 * row + 1] = s;
    }
    const float rinv = 1.0f / s;
    if (one) {
#pragma unroll
        for (int i = 0; i < NS; ++i) z[i] = z[i] * rinv;
        attn_store<DT, ATTN_NT_STORE != 0, G>(a.y, base, 0, a.cols, lane, z);
    } else {
        for (int64_t c0 = 0; c0 < a.cols; c0 += G::SWEEP) {
            float t[NS];
            attn_a_sweep<DT, MDT, G>(a.x, a.m.p, base, mbase, c0, a.cols, lane, a.inv, t);
            attn_z_slots<DT, MDT, G>(t, c0, a.cols, lane);
#pragma unroll
            for (int i = 0; i < NS; ++i) t[i] = attn_p(t[i], ref, rinv);
            attn_store<DT, ATTN_NT_STORE != 0, G>(a.y, base, c0, a.cols, lane, t);
        }
    }
}

// one sweep of the backward: a (in front of the clamp), p (0 past the row) and g -> the lane's part of sum(g p) in slot order
template <int DT, int MDT, class G>
__device__ __forceinline__ float attn_bwd_sweep(const AttnBwdArgs& k, int64_t base, int64_t mbase, int64_t c0, int lane, float ref, float rinv,
                                                float (&a)[G::NS], float (&p)[G::NS], float (&g)[G::NS]) {
    attn_a_sweep<DT, MDT, G>(k.x, k.m.p, base, mbase, c0, k.cols, lane, k.inv, a);
    attn_load<DT, ATTN_NT_LOAD != 0, G>(k.g, base, c0, k.cols, lane, g);
    float dot = 0.0f;
#pragma unroll
    for (int i = 0; i < G::NG; ++i) {
        const bool in = G::in(i, c0, k.cols, lane);
#pragma unroll
        for (int e = 0; e < G::EPV; ++e) {
            const int s = i * G::EPV + e;
            p[s] = attn_p(in ? attn_z<DT, MDT>(a[s]) : LOSS_NEG_INF, ref, rinv);
            g[s] = in ? g[s] : 0.0f;
            dot += g[s] * p[s];
        }
    }
    return dot;
}
// dx's slots into g: d = (g - dot) p, rounded to P; the gradient of max(a, MIN_P); rounded to the dtype; times inv (the store rounds)
template <int DT, int MDT, int N> __device__ __forceinline__ void attn_dx(float (&g)[N], const float (&p)[N], const float (&a)[N], float dot, float inv) {
    constexpr int P = attn_sum_dtype<DT, MDT>();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float d = (g[i] - dot) * p[i];
        if constexpr (P == F16) asm("" : "+v"(d));
        d = Ty<P>::rb(d);
        if constexpr (MDT != ATTN_NOMASK) {
            const float mn = attn_min<P>();
            const float h = Ty<P>::rb(d * 0.5f);
            d = a[i] == mn ? h : (a[i] < mn ? 0.0f : d);      // a NaN a compares false twice: d passes
        }
        float o = Ty<DT>::rb(d) * inv;
        if constexpr (DT == F16) asm("" : "+v"(o));
        g[i] = o;
    }
}

template <int DT, int MDT, bool VEC, int TPR, int NGV>
__global__ __launch_bounds__(ROW_TPB) void attn_bwd_kernel(AttnBwdArgs k) {
    using G = AttnGeom<DT, VEC, TPR, NGV>;
    constexpr int NS = G::NS, NW = TPR / 64;
    __shared__ uint32_t lds[1][4];
    int64_t row;
    int lane;
    if (!row_lane<TPR>(k.rows, row, lane)) return;
    const int64_t base = row * k.cols;
    const int64_t mbase = attn_mask_base<MDT>(k.m, row, k.rows);
    const float ref = loss_ref(k.stats[2 * row]);
    const float rinv = 1.0f / k.stats[2 * row + 1];
    if (k.cols <= G::SWEEP) {
        float a[NS], p[NS], g[NS];
        uint32_t v[1] = {as_u(attn_bwd_sweep<DT, MDT, G>(k, base, mbase, 0, lane, ref, rinv, a, p, g))};
        row_reduce<OpAddF, NW>(v, lds);
        attn_dx<DT, MDT>(g, p, a, as_f(v[0]), k.inv);
        attn_store<DT, ATTN_NT_STORE != 0, G>(k.dx, base, 0, k.cols, lane, g);
    } else {
        float dot = 0.0f;
        for (int64_t c0 = 0; c0 < k.cols; c0 += G::SWEEP) {
            float a[NS], p[NS], g[NS];
            dot += attn_bwd_sweep<DT, MDT, G>(k, base, mbase, c0, lane, ref, rinv, a, p, g);
        }
        uint32_t v[1] = {as_u(dot)};
        row_reduce<OpAddF, NW>(v, lds);
        for (int64_t c0 = 0; c0 < k.cols; c0 += G::SWEEP) {
            float a[NS], p[NS], g[NS];
            attn_bwd_sweep<DT, MDT, G>(k, base, mbase, c0, lane, ref, rinv, a, p, g);
            attn_dx<DT, MDT>(g, p, a, as_f(v[0]), k.inv);
            attn_store<DT, ATTN_NT_STORE != 0, G>(k.dx, base, c0, k.cols, lane, g);
        }
    }
}

// the most 16-byte vectors of a lane per sweep and the three counts a kernel is built for (as fq_rms_norm.h): 8, 16 or 32 slots
template <int DT> constexpr int attn_most_groups() { return ATTN_VIF * Ty<DT>::ESIZE / 2; }
constexpr int attn_groups(int most, int step) { return (most >> step) > 0 ? most >> step : 1; }

}  // namespace fq
