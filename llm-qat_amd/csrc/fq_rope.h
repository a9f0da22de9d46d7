// fq_rope.h -- the rotary position embedding of q and k and its gradient: the kernels behind
// include/llmqat_fakequant_rope.h.  One streaming kernel, forward or backward, serves q and k in one launch: fp32 arithmetic in the op
// order of the eager chain  x * cos + rotate_half(x) * sin  and of its autograd, with the chain's roundings, so the results are the
// chain's bit for bit.  It stands on the row layer of fq_rows.h (unpack / pack, the workgroup size) and the launch helper of fq_launch.h.
//
//   rope_kernel<DT, VEC, TF32, BWD>   a workgroup owns one token (b, t): it reads the position once, and its lanes walk the items of the
//                                     token, ROW_TPB at a time.  An item is one group of the first half of one head of q or of k together
//                                     with the matching group of the second half, so both partners of the rotation are in the same lane.
//                                     The heads of q come first, then those of k.  ROPE_IIF items of a lane are loaded before the first is
//                                     used.  Where a head's groups divide the workgroup (every power of two up to 256: D = 128 in bf16 is 8)
//                                     a lane meets the same group of every head, and its cos / sin values are loaded once.
//
// 16-byte path (VEC): a group is one 16-byte vector; element path (any even D, an offset base, an odd stride): one element.  Both feed the
// same arithmetic.  TF32: the tables are fp32 and are rounded to DT here, as the chain's .to(dtype) does; else they are DT.  BWD: x is the
// incoming gradient and the rotation runs the other way (rope_bwd).  A side with no heads (H = 0: the backward of a frozen q or k) has no
// items: it is neither read, computed nor stored.
//
// A position p in [-P, 0) wraps to p + P; one outside [-P, P) reads the table's row 0 instead of a row that does not exist, and its cos
// and sin are NaN: so is every output of the token.
//
// What the compiler must not fold: a product and the sum behind it into an fma (any dtype: the chain stores each product; the build's
// -ffp-contract=off), and for fp16 a product and its conversion into v_fma_mixlo_f16 (swi_prod's barrier, fq_swiglu.h).
// ROPE_NT_LOAD / ROPE_NT_STORE: cache policies of the 16-byte streams; ROPE_IIF: items of a lane in flight.  A/B macros as SWIGLU_* are; the A/B is
// profiles/rope_ab.txt.  rope_token / rope_item: the walk that rope_kernel and rope_mixed_kernel share.
#pragma once
#include "fq_rows.h"
#include "fq_swiglu.h"   // swi_prod

#ifndef ROPE_NT_LOAD
#define ROPE_NT_LOAD 0       // q and k were written by the projections just before; non-temporal measured no faster
#endif
#ifndef ROPE_NT_STORE
#define ROPE_NT_STORE 0      // the attention product reads the results next; non-temporal measured within the spread
#endif
#ifndef ROPE_IIF
#define ROPE_IIF 1           // one item: two 16-byte vectors of a lane in flight; measured against 2 and 4
#endif

namespace fq {

struct RopeSide {
    const void* x;        // forward: q or k; backward: the gradient of its embedding
    void* y;              // forward: the embedding; backward: the gradient
    int64_t xs[3];        // element strides of x over batch, head, token (the last stride is 1)
    int64_t ys[3];        // the same of y: dense in x's dimension order
    int32_t H;            // heads; 0: no such side in this launch
    int32_t narrow;       // rope_mixed_kernel: this side's tensor (forward: x, backward: y) is the 16-bit one
};

struct RopeArgs {
    RopeSide s[2];
    const void* cos;      // [P, 2 h], rows contiguous
    const void* sin;
    const int64_t* pos;   // [B, T] or [1, T]; nullptr: the token index
    int64_t pos_bs;       // elements between two batches of pos: T or 0
    int64_t P, T;
    int32_t h;            // D / 2
};

template <int DT, bool VEC, bool TF32> struct RopeIO {
    using T = Ty<DT>;
    static constexpr int EPV = VEC ? 16 / T::ESIZE : 1;
    using Raw = std::conditional_t<VEC, uint4, float>;

    __device__ static __forceinline__ Raw load(const void* p, int64_t at) {
        if constexpr (VEC) return ld16<ROPE_NT_LOAD != 0>((const uint4*)((const char*)p + at * T::ESIZE));
        else return T::load1(p, at);
    }
    __device__ static __forceinline__ void unpack(const Raw& r, float (&e)[EPV]) {
        if constexpr (VEC) row_unpack<DT>(r, e);
        else e[0] = r;
    }
    __device__ static __forceinline__ void store(void* p, int64_t at, const float (&e)[EPV]) {
        if constexpr (VEC) st16<ROPE_NT_STORE != 0>((uint4*)((char*)p + at * T::ESIZE), row_pack<DT>(e));
        else T::store1(p, at, e[0]);
    }
    // EPV table values from element `at`, rounded to DT
    __device__ static __forceinline__ void table(const void* p, int64_t at, float (&e)[EPV]) {
        if constexpr (!TF32) {
            unpack(load(p, at), e);
        } else if constexpr (VEC) {
#pragma unroll
            for (int v = 0; v < EPV / 4; ++v) {
                const uint4 r = *((const uint4*)((const char*)p + at * 4) + v);
                e[v * 4 + 0] = T::rb(as_f(r.x));
                e[v * 4 + 1] = T::rb(as_f(r.y));
                e[v * 4 + 2] = T::rb(as_f(r.z));
                e[v * 4 + 3] = T::rb(as_f(r.w));
            }
        } else {
            e[0] = T::rb(((const float*)p)[at]);
        }
    }
};

// forward of one element pair: y1 = rb(x1 c1) + rb(-x2 s1), y2 = rb(x2 c2) + rb(x1 s2); the store rounds the sums
template <int DT> __device__ __forceinline__ void rope_fwd(float x1, float x2, float c1, float c2, float s1, float s2, float& y1, float& y2) {
    using T = Ty<DT>;
    y1 = T::rb(swi_prod<DT>(x1, c1)) + T::rb(swi_prod<DT>(-x2, s1));
    y2 = T::rb(swi_prod<DT>(x2, c2)) + T::rb(swi_prod<DT>(x1, s2));
}
// backward: a = rb(g c), b = rb(g s); dx1 = rb(a1 + b2) + 0, dx2 = rb(a2 - b1) + 0.  The + 0 is autograd's sum of the zero-padded slice
// gradients: a zero comes out as +0
template <int DT> __device__ __forceinline__ void rope_bwd(float g1, float g2, float c1, float c2, float s1, float s2, float& d1, float& d2) {
    using T = Ty<DT>;
    const float a1 = T::rb(swi_prod<DT>(g1, c1)), a2 = T::rb(swi_prod<DT>(g2, c2));
    const float b1 = T::rb(swi_prod<DT>(g1, s1)), b2 = T::rb(swi_prod<DT>(g2, s2));
    d1 = T::rb(a1 + b2) + 0.0f;
    d2 = T::rb(a2 + (-b1)) + 0.0f;
}

// ---- the walk that both kernels share ---------------------------------------------------------------------------------------------------
// the token of a workgroup: its batch and token index, its table row, whether its position lies in the table, and its items
struct RopeToken {
    int64_t b, t, trow;
    bool in;
    uint32_t L, H0, items;
};
template <int EPV> __device__ __forceinline__ RopeToken rope_token(const RopeArgs& a) {
    RopeToken k;
    k.b = blockIdx.x / a.T;
    k.t = blockIdx.x - k.b * a.T;
    int64_t p = a.pos ? a.pos[k.b * a.pos_bs + k.t] : k.t;
    if (p < 0) p += a.P;
    k.in = p >= 0 && p < a.P;
    k.trow = (k.in ? p : 0) * 2 * a.h;                     // the position's table row; a position outside the table reads row 0 ...
    k.L = (uint32_t)(a.h / EPV);                           // groups (lanes) of a head
    k.H0 = (uint32_t)a.s[0].H;
    k.items = (k.H0 + (uint32_t)a.s[1].H) * k.L;
    return k;
}
// ... and its table values become NaN
template <int EPV> __device__ __forceinline__ void rope_outside(bool in, float (&c1)[EPV], float (&c2)[EPV], float (&s1)[EPV], float (&s2)[EPV]) {
    const float nan = as_f(0x7FC00000u);
#pragma unroll
    for (int k = 0; k < EPV; ++k) {
        c1[k] = in ? c1[k] : nan;
        c2[k] = in ? c2[k] : nan;
        s1[k] = in ? s1[k] : nan;
        s2[k] = in ? s2[k] : nan;
    }
}
// item `it` of the token: its tensors, the element offsets of its first-half group in them, its group of the head, its side's flag
struct RopeItem {
    const void* x;
    void* y;
    int64_t xat, yat;
    uint32_t j;
    bool narrow;
};
template <int EPV> __device__ __forceinline__ RopeItem rope_item(const RopeArgs& a, const RopeToken& k, uint32_t it) {
    const uint32_t head = it / k.L;
    const bool side = head >= k.H0;
    const int64_t hh = side ? head - k.H0 : head;
    RopeItem m;
    m.j = it - head * k.L;
    m.x = side ? a.s[1].x : a.s[0].x;
    m.y = side ? a.s[1].y : a.s[0].y;
    m.narrow = (side ? a.s[1].narrow : a.s[0].narrow) != 0;
    m.xat = k.b * (side ? a.s[1].xs[0] : a.s[0].xs[0]) + hh * (side ? a.s[1].xs[1] : a.s[0].xs[1]) + k.t * (side ? a.s[1].xs[2] : a.s[0].xs[2]) +
            (int64_t)m.j * EPV;
    m.yat = k.b * (side ? a.s[1].ys[0] : a.s[0].ys[0]) + hh * (side ? a.s[1].ys[1] : a.s[0].ys[1]) + k.t * (side ? a.s[1].ys[2] : a.s[0].ys[2]) +
            (int64_t)m.j * EPV;
    return m;
}

template <int DT, bool VEC, bool TF32, bool BWD>
__global__ __launch_bounds__(ROW_TPB) void rope_kernel(RopeArgs a) {
    using IO = RopeIO<DT, VEC, TF32>;
    constexpr int EPV = IO::EPV;
    const RopeToken tk = rope_token<EPV>(a);

    float c1[EPV], c2[EPV], s1[EPV], s2[EPV];                       // the lane's table groups: cos and sin of the first and of the second half
    auto load_cs = [&](uint32_t j) {
        const int64_t at = tk.trow + (int64_t)j * EPV;
        IO::table(a.cos, at, c1);
        IO::table(a.cos, at + a.h, c2);
        IO::table(a.sin, at, s1);
        IO::table(a.sin, at + a.h, s2);
        rope_outside<EPV>(tk.in, c1, c2, s1, s2);
    };
    const bool fixed = ROW_TPB % tk.L == 0;                         // a lane meets one group of every head
    if (fixed) load_cs(threadIdx.x % tk.L);

    for (uint32_t i0 = threadIdx.x; i0 < tk.items; i0 += ROW_TPB * ROPE_IIF) {
        typename IO::Raw lo[ROPE_IIF], hi[ROPE_IIF];
        RopeItem m[ROPE_IIF];
#pragma unroll
        for (int n = 0; n < ROPE_IIF; ++n) {
            const uint32_t it = i0 + n * ROW_TPB;
            m[n] = rope_item<EPV>(a, tk, it < tk.items ? it : i0);  // an item past the token re-reads the lane's first and is not stored
            if (it >= tk.items) m[n].y = nullptr;
            lo[n] = IO::load(m[n].x, m[n].xat);
            hi[n] = IO::load(m[n].x, m[n].xat + a.h);
        }
#pragma unroll
        for (int n = 0; n < ROPE_IIF; ++n) {
            if (!fixed) load_cs(m[n].j);
            float x1[EPV], x2[EPV];
            IO::unpack(lo[n], x1);
            IO::unpack(hi[n], x2);
#pragma unroll
            for (int k = 0; k < EPV; ++k) {
                float y1, y2;
                if constexpr (BWD) rope_bwd<DT>(x1[k], x2[k], c1[k], c2[k], s1[k], s2[k], y1, y2);
                else rope_fwd<DT>(x1[k], x2[k], c1[k], c2[k], s1[k], s2[k], y1, y2);
                x1[k] = y1;
                x2[k] = y2;
            }
            if (m[n].y) {
                IO::store(m[n].y, m[n].yat, x1);
                IO::store(m[n].y, m[n].yat + a.h, x2);
            }
        }
    }
}

// ---- q and k in two dtypes: one of them DT16, the other fp32, the tables fp32 --------------------------------------------------------------
// The chain promotes: its products x * cos and rotate_half(x) * sin are fp32 tensors for both sides, so the forward is rope_fwd<F32> on
// the 16-bit side's values and its result is fp32; the incoming gradients are fp32, and autograd rounds the two products g * cos and
// g * sin to the 16-bit tensor's dtype before it sums the slices in that dtype: rope_bwd<DT16> on fp32 gradients, the result 16-bit.  The
// fp32 side is rope_fwd<F32> / rope_bwd<F32>.  The tables are used as they are.  The walk is rope_kernel's; a group is 8 elements on the
// 16-byte path (one vector of the 16-bit tensor, two of an fp32 one) and one element otherwise.
template <int DT16, bool VEC> struct RopeMixIO {
    static constexpr int EPV = VEC ? 8 : 1;
    __device__ static __forceinline__ void load(const void* p, int64_t at, bool narrow, float (&e)[EPV]) {
        if constexpr (VEC) {
            if (narrow) {
                row_unpack<DT16>(ld16<ROPE_NT_LOAD != 0>((const uint4*)((const char*)p + at * 2)), e);
            } else {
#pragma unroll
                for (int v = 0; v < 2; ++v) {
                    const uint4 r = ld16<ROPE_NT_LOAD != 0>((const uint4*)((const char*)p + at * 4) + v);
                    e[v * 4 + 0] = as_f(r.x), e[v * 4 + 1] = as_f(r.y), e[v * 4 + 2] = as_f(r.z), e[v * 4 + 3] = as_f(r.w);
                }
            }
        } else {
            e[0] = narrow ? Ty<DT16>::load1(p, at) : ((const float*)p)[at];
        }
    }
    __device__ static __forceinline__ void store(void* p, int64_t at, bool narrow, const float (&e)[EPV]) {
        if constexpr (VEC) {
            if (narrow) {
                st16<ROPE_NT_STORE != 0>((uint4*)((char*)p + at * 2), row_pack<DT16>(e));
            } else {
#pragma unroll
                for (int v = 0; v < 2; ++v)
                    st16<ROPE_NT_STORE != 0>((uint4*)((char*)p + at * 4) + v, make_uint4(as_u(e[v * 4 + 0]), as_u(e[v * 4 + 1]), as_u(e[v * 4 + 2]), as_u(e[v * 4 + 3])));
            }
        } else {
            if (narrow) Ty<DT16>::store1(p, at, e[0]);
            else ((float*)p)[at] = e[0];
        }
    }
};

template <int DT16, bool VEC, bool BWD>
__global__ __launch_bounds__(ROW_TPB) void rope_mixed_kernel(RopeArgs a) {
    using IO = RopeMixIO<DT16, VEC>;
    constexpr int EPV = IO::EPV;
    const RopeToken tk = rope_token<EPV>(a);

    float c1[EPV], c2[EPV], s1[EPV], s2[EPV];
    auto load_cs = [&](uint32_t j) {
        const int64_t at = tk.trow + (int64_t)j * EPV;
        IO::load(a.cos, at, false, c1);
        IO::load(a.cos, at + a.h, false, c2);
        IO::load(a.sin, at, false, s1);
        IO::load(a.sin, at + a.h, false, s2);
        rope_outside<EPV>(tk.in, c1, c2, s1, s2);
    };
    const bool fixed = ROW_TPB % tk.L == 0;
    if (fixed) load_cs(threadIdx.x % tk.L);

    for (uint32_t it = threadIdx.x; it < tk.items; it += ROW_TPB) {      // (one item of a lane in flight: this kernel has no ROPE_IIF)
        const RopeItem m = rope_item<EPV>(a, tk, it);
        float x1[EPV], x2[EPV];
        IO::load(m.x, m.xat, !BWD && m.narrow, x1);         // forward: the 16-bit tensor is read; backward: it is written
        IO::load(m.x, m.xat + a.h, !BWD && m.narrow, x2);
        if (!fixed) load_cs(m.j);
        if (BWD && m.narrow) {                              // the 16-bit side's gradient: that dtype's roundings
#pragma unroll
            for (int e = 0; e < EPV; ++e) rope_bwd<DT16>(x1[e], x2[e], c1[e], c2[e], s1[e], s2[e], x1[e], x2[e]);
        } else {
#pragma unroll
            for (int e = 0; e < EPV; ++e) {
                if constexpr (BWD) rope_bwd<F32>(x1[e], x2[e], c1[e], c2[e], s1[e], s2[e], x1[e], x2[e]);
                else rope_fwd<F32>(x1[e], x2[e], c1[e], c2[e], s1[e], s2[e], x1[e], x2[e]);
            }
        }
        IO::store(m.y, m.yat, BWD && m.narrow, x1);
        IO::store(m.y, m.yat + a.h, BWD && m.narrow, x2);
    }
}

}  // namespace fq
