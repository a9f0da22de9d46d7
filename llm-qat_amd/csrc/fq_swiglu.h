// fq_swiglu.h -- the gated activation  y = silu(gate) * up  of a LLaMA MLP and its gradients: the kernels behind
// include/llmqat_fakequant_act.h.  Two streaming kernels without a reduction: fp32 arithmetic in the op order of the eager chain
// F.silu(gate) * up and of its autograd, with the chain's roundings, so the results are the chain's bit for bit.  They stand on the row
// layer of fq_rows.h (unpack / pack, the workgroup size) and the launch helper of fq_launch.h.
//
//   swiglu_fwd_kernel   a workgroup owns one tile of one row of the walk: SwiIO::TILE consecutive columns.  A lane loads its groups of gate
//                       and of up (all of them before the first is used: SWIGLU_VIF = 2 16-byte vectors per tensor in flight), then
//                       computes and stores group by group.
//   swiglu_bwd_kernel   the same walk over dy, gate and up.  <DG, DU>: which of dgate and dup is wanted; the other one's arithmetic and
//                       store are not in the kernel, and without dgate up is not read.
//
// The walk: the tensors are [rows, cols] with a row stride each; where every stride equals cols the host hands the kernel one row of
// rows * cols columns (the flat walk, no tail per row), else rows of cols columns (the row-wise walk, a tail tile per row).  A workgroup
// finds its row by one division of its index by the tiles of a row.  16-byte path (SwiIO<DT, true>): group i of a lane is vector
// i * 256 + lane of the tile; element path (any cols, an offset base, an odd stride): element i * 256 + lane.  Both feed the same
// arithmetic.  A group past the end of the row re-reads the tile's first (whose values are harmless) and is not stored.
//
// What the compiler must not fold (fp16): left alone, a product and the conversion behind it become one v_fma_mixlo_f16(a, b, +0), which
// section 25 found to change tie rounding and to lose the sign of a zero product.  An empty asm keeps each product that is rounded to the
// dtype in an fp32 register of its own; with it every fp16 result equals the chain's but for the sign of a zero dg in the remainder of
// ATen's own loop (swi_dgate).
// SWIGLU_NT_LOAD / SWIGLU_NT_STORE: cache policies of the 16-byte streams; SWIGLU_VIF / SWIGLU_EIF: 16-byte vectors / elements of one
// tensor a lane holds; SWIGLU_BWD_FMA: 1 + g (1 - sig) as one fma, as ATen's device code has it (0: a product and a sum).  A/B macros as
// RMS_* are.
#pragma once
#include <cmath>

#include "fq_rows.h"

#ifndef SWIGLU_NT_LOAD
#define SWIGLU_NT_LOAD 0      // gate and up were written by the GEMMs just before, and the backward reads them again
#endif
#ifndef SWIGLU_NT_STORE
#define SWIGLU_NT_STORE 1     // as the norm's and the losses' outputs: a plain store leaves the lines dirty in the caches
#endif
#ifndef SWIGLU_VIF
#define SWIGLU_VIF 2         // measured against 1, 4 and 8
#endif
#ifndef SWIGLU_EIF
#define SWIGLU_EIF 8
#endif
#ifndef SWIGLU_BWD_FMA
#define SWIGLU_BWD_FMA 1
#endif

namespace fq {

struct SwiGluArgs {
    const void* dy;       // the backward's
    const void* g;
    const void* u;
    void* o0;             // forward: y; backward: dgate or nullptr
    void* o1;             // backward: dup or nullptr
    int64_t cols;         // columns of a row of the walk
    int64_t sdy, sg, su;  // row strides in elements (the outputs': cols)
    uint32_t tpr;         // tiles of a row: the grid is rows * tpr
};

template <int DT, bool VEC> struct SwiIO {
    using T = Ty<DT>;
    static constexpr int EPV = VEC ? 16 / T::ESIZE : 1;                     // elements of a group
    static constexpr int NG = VEC ? SWIGLU_VIF : SWIGLU_EIF;                // groups of a lane
    static constexpr int64_t TILE = (int64_t)NG * EPV * ROW_TPB;            // columns of a workgroup
    using Raw = std::conditional_t<VEC, uint4, float>;

    // the lane's groups of the tile that starts at column c0 (< cols) of the row that starts at element `base` of p
    template <bool NT> __device__ static __forceinline__ void load(const void* p, int64_t base, int64_t c0, int64_t cols, Raw (&r)[NG]) {
        const int64_t n = (cols - c0) / EPV;
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int64_t gi = (int64_t)i * ROW_TPB + threadIdx.x;
            const int64_t at = gi < n ? gi : 0;
            if constexpr (VEC) r[i] = ld16<NT>((const uint4*)((const char*)p + (base + c0) * T::ESIZE) + at);
            else r[i] = T::load1(p, base + c0 + at);
        }
    }
    __device__ static __forceinline__ void unpack(const Raw& r, float (&e)[EPV]) {
        if constexpr (VEC) row_unpack<DT>(r, e);
        else e[0] = r;
    }
    // group i back, rounded once to DT; a group past the row is not stored
    template <bool NT> __device__ static __forceinline__ void store(void* p, int64_t base, int64_t c0, int64_t cols, int i, const float (&e)[EPV]) {
        const int64_t gi = (int64_t)i * ROW_TPB + threadIdx.x;
        if (gi < (cols - c0) / EPV) {
            if constexpr (VEC) st16<NT>((uint4*)((char*)p + (base + c0) * T::ESIZE) + gi, row_pack<DT>(e));
            else T::store1(p, base + c0 + gi, e[0]);
        }
    }
    // the workgroup's row of the walk and its tile's first column
    __device__ static __forceinline__ void place(uint32_t tpr, int64_t& row, int64_t& c0) {
        const uint32_t r = blockIdx.x / tpr;
        row = r;
        c0 = (int64_t)(blockIdx.x - r * tpr) * TILE;
    }
};

// a product that the dtype rounds next, kept an fp32 product (see the head of this file)
template <int DT> __device__ __forceinline__ float swi_prod(float a, float b) {
    float p = a * b;
    if constexpr (DT == F16) asm("" : "+v"(p));
    return p;
}
// 1 + exp(-g): the denominator of silu and of the sigmoid
__device__ __forceinline__ float swi_den(float g) { return 1.0f + expf(-g); }
// rb(silu(g)): ATen's x / (1 + exp(-x)), rounded as the chain stores it
template <int DT> __device__ __forceinline__ float swi_act(float g, float den) { return Ty<DT>::rb(g / den); }
// ATen's silu_backward on the rounded ds: ds * sig * (1 + g * (1 - sig))
template <int DT> __device__ __forceinline__ float swi_dgate(float ds, float g, float den) {
    const float sig = 1.0f / den;
#if SWIGLU_BWD_FMA
    const float t = __builtin_fmaf(g, 1.0f - sig, 1.0f);
#else
    const float t = 1.0f + g * (1.0f - sig);
#endif
    // (fp16: the chain's own sign of a zero dg depends on where ATen's kernel meets the element.  In the remainder behind the last whole
    // block of 4096 elements of its loop a product of -0 is stored as +0, which is what an fma with a +0 addend gives; in the whole blocks it
    // stays -0, as in the bf16 and fp32 chains.  This kernel keeps the product's own sign everywhere: DESIGN.md section 27)
    return swi_prod<DT>(ds * sig, t);
}

template <int DT, bool VEC>
__global__ __launch_bounds__(ROW_TPB) void swiglu_fwd_kernel(SwiGluArgs a) {
    using IO = SwiIO<DT, VEC>;
    int64_t row, c0;
    IO::place(a.tpr, row, c0);
    typename IO::Raw rg[IO::NG], ru[IO::NG];
    IO::template load<SWIGLU_NT_LOAD != 0>(a.g, row * a.sg, c0, a.cols, rg);
    IO::template load<SWIGLU_NT_LOAD != 0>(a.u, row * a.su, c0, a.cols, ru);
#pragma unroll
    for (int i = 0; i < IO::NG; ++i) {
        float g[IO::EPV], u[IO::EPV];
        IO::unpack(rg[i], g);
        IO::unpack(ru[i], u);
#pragma unroll
        for (int k = 0; k < IO::EPV; ++k) g[k] = swi_prod<DT>(swi_act<DT>(g[k], swi_den(g[k])), u[k]);
        IO::template store<SWIGLU_NT_STORE != 0>(a.o0, row * a.cols, c0, a.cols, i, g);
    }
}

template <int DT, bool VEC, bool DG, bool DU>
__global__ __launch_bounds__(ROW_TPB) void swiglu_bwd_kernel(SwiGluArgs a) {
    using IO = SwiIO<DT, VEC>;
    static_assert(DG || DU, "one gradient at least");
    int64_t row, c0;
    IO::place(a.tpr, row, c0);
    typename IO::Raw rd[IO::NG], rg[IO::NG], ru[DG ? IO::NG : 1];
    IO::template load<SWIGLU_NT_LOAD != 0>(a.dy, row * a.sdy, c0, a.cols, rd);
    IO::template load<SWIGLU_NT_LOAD != 0>(a.g, row * a.sg, c0, a.cols, rg);
    if constexpr (DG) IO::template load<SWIGLU_NT_LOAD != 0>(a.u, row * a.su, c0, a.cols, ru);
#pragma unroll
    for (int i = 0; i < IO::NG; ++i) {
        float d[IO::EPV], g[IO::EPV], dg[IO::EPV], du[IO::EPV];
        IO::unpack(rd[i], d);
        IO::unpack(rg[i], g);
        if constexpr (DG) IO::unpack(ru[i], dg);            // up's values, until dgate's replace them
#pragma unroll
        for (int k = 0; k < IO::EPV; ++k) {
            const float den = swi_den(g[k]);
            if constexpr (DU) du[k] = swi_prod<DT>(d[k], swi_act<DT>(g[k], den));
            if constexpr (DG) dg[k] = swi_dgate<DT>(Ty<DT>::rb(swi_prod<DT>(d[k], dg[k])), g[k], den);
        }
        if constexpr (DG) IO::template store<SWIGLU_NT_STORE != 0>(a.o0, row * a.cols, c0, a.cols, i, dg);
        if constexpr (DU) IO::template store<SWIGLU_NT_STORE != 0>(a.o1, row * a.cols, c0, a.cols, i, du);
    }
}

}  // namespace fq
