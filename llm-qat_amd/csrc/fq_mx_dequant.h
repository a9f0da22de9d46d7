// fq_mx_dequant.h -- an MX export back to a tensor in one launch: the element codes and E8M0 scale bytes that
// mx_kernel<DT, MX_EXP4 / MX_EXP8> (fq_mx.h) writes, expanded to bf16 / fp16 / fp32.  The inverse walk of that kernel's export arm:
//
//   mx_dequant_kernel   a contiguous export is a flat sequence of blocks.  Lane t of workgroup b owns the 16-byte OUTPUT vectors
//                       b * TPB * VPT + i * TPB + t (VPT of them in flight, mx_rows_grid workgroups).  Vector v holds EPV = 16 / esize
//                       elements of one block: its codes are the EPV / 2 (fp4) or EPV (fp8) bytes at elems + v * that many, its scale is
//                       byte v / BV (BV = 32 / EPV vectors per block).  A wave's code loads and its stores are one contiguous run per
//                       instruction; the scale byte is read by each of the block's BV lanes (one line, served from the cache).
//                       Slots past the end re-load the last vector and are not stored.  No LDS, no barrier.
//
// Semantics (ops.MXExport.dequantize, bit for bit):
//   q   the OCP value of the code, exact in fp32.  The code's magnitude bits are shifted to the top of an fp32's exponent / mantissa
//       field: that fp32 is q * 2^-(127 - bias), a normal code a normal, a subnormal code a subnormal with the same mantissa bits, so one
//       multiply by 2^(127 - bias) (exact) rebiases both.  FP4 E2M1 (bias 1): sign in bit 3, element 2k in the low nibble of byte k.
//       FP8: float8_e4m3fn (bias 7; S.1111.111 is NaN, no Inf) and float8_e5m2 (bias 15; exponent 31: Inf / NaN), selected on the bits.
//   s   2^(byte - 127) from its fp32 bits; byte 0 is 2^-127, the subnormal 0x00400000; byte 0xFF is NaN, so the block's 32 outputs are.
//   y   q * s, one fp32 multiply: exact or +-Inf (q has at most 4 significant bits and q * s >= 2^-143), fp32 subnormals kept; then
//       rounded once, nearest-even, to the dtype (Ty<DT>::pack), gradual underflow included.  -0 stays -0: the sign rides in the bits.
//
// Cache policy.  The codes are read once: non-temporal loads (MXD_NT_LOAD).  The output is read by the GEMM that follows, so its store
// policy was measured on the layer's time, not assumed (MXD_NT_STORE; DESIGN.md section 21 has the figures).  Both are macros so that an
// A/B build of the library (build.py extra_flags) differs in nothing else.
#pragma once
#include "fq_mx.h"

#ifndef MXD_NT_LOAD
#define MXD_NT_LOAD 1
#endif
#ifndef MXD_NT_STORE
#define MXD_NT_STORE 1
#endif

namespace fq {

enum : int { MXD_FP4 = 0, MXD_FP8 = 1 };

// the CB code bytes of one output vector (2, 4 or 8): one load
template <int CB> __device__ __forceinline__ void mxd_load_codes(const uint8_t* p, uint32_t (&c)[2]) {
    c[1] = 0;
    if constexpr (CB == 8) {
        const u32x2_t* q = (const u32x2_t*)p;
        const u32x2_t v = MXD_NT_LOAD ? __builtin_nontemporal_load(q) : *q;
        c[0] = v.x, c[1] = v.y;
    } else if constexpr (CB == 4) {
        const uint32_t* q = (const uint32_t*)p;
        c[0] = MXD_NT_LOAD ? __builtin_nontemporal_load(q) : *q;
    } else {
        const uint16_t* q = (const uint16_t*)p;
        c[0] = MXD_NT_LOAD ? __builtin_nontemporal_load(q) : *q;
    }
}

// fp32 bits of the block's scale from its E8M0 byte
__device__ __forceinline__ float mxd_scale(uint32_t b) {
    const uint32_t u = b == 0u ? 0x00400000u : (b == 0xFFu ? 0x7FC00000u : b << 23);
    return as_f(u);
}

// q of one FP4 code (4 bits) / one FP8 code (8 bits), exact in fp32
__device__ __forceinline__ float mxd_fp4(uint32_t c) {
    return as_f(((c & 8u) << 28) | ((c & 7u) << 22)) * 0x1p126f;
}
template <bool E5M2> __device__ __forceinline__ float mxd_fp8(uint32_t c) {
    const uint32_t sign = (c & 0x80u) << 24, mag = c & 0x7Fu;
    if constexpr (E5M2) {
        const float q = as_f(sign | (mag << 21)) * 0x1p112f;
        return mag >= 0x7Cu ? as_f(sign | 0x7F800000u | ((mag & 3u) << 21)) : q;     // exponent 31: Inf, or NaN with its mantissa bits
    } else {
        const float q = as_f(sign | (mag << 20)) * 0x1p120f;
        return mag == 0x7Fu ? as_f(0x7FC00000u) : q;
    }
}

template <int DT, int KIND, bool E5M2, int VPT>
__global__ __launch_bounds__(MX_TPB) void mx_dequant_kernel(MxDequantArgs a) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE;                       // elements per output vector
    constexpr int BV = 32 / EPV;                             // vectors per block
    constexpr int CB = KIND == MXD_FP4 ? EPV / 2 : EPV;      // code bytes per output vector
    static_assert(KIND == MXD_FP8 || !E5M2, "the FP8 flavour belongs to the FP8 codes");
    const int64_t base = (int64_t)blockIdx.x * (MX_TPB * VPT) + threadIdx.x;

    // Out-of-range slots re-load the last vector's codes and scale and are never stored (nvec > 0: the entry point's check).
    uint32_t c[VPT][2], sb[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t v = base + i * MX_TPB, vc = v < a.nvec ? v : a.nvec - 1;
        mxd_load_codes<CB>(a.elems + vc * CB, c[i]);
        sb[i] = a.scales[(uint64_t)vc / BV];
    }
    // every load is issued here: without the first the first slot's loads are sunk behind its store's branch, without the second the
    // scheduler lifts that slot's arithmetic (and the wait for its loads) above the other slots' loads
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t v = base + i * MX_TPB;
        const float s = mxd_scale(sb[i]);
        uint32_t o[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            float fd[T::EPD];
#pragma unroll
            for (int k = 0; k < T::EPD; ++k) {
                const int e = d * T::EPD + k;                // element of the vector
                float q;
                if constexpr (KIND == MXD_FP4) q = mxd_fp4(c[i][0] >> (4 * e));
                else q = mxd_fp8<E5M2>(c[i][e >> 2] >> (8 * (e & 3)));
                fd[k] = q * s;
            }
            o[d] = T::pack(fd);
        }
        asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]));   // computed for every lane: only the store is predicated
        if (v < a.nvec) st16<MXD_NT_STORE != 0>(&((uint4*)a.y)[v], make_uint4(o[0], o[1], o[2], o[3]));
    }
}

// a validated by fqi_mx_dequant (fq_api.hip): nvec > 0, grid within limits; fmt one of FQ_MX_FP4_E2M1 / FP8_E4M3 / FP8_E5M2
template <int DT> int launch_mx_dequant(int fmt, MxDequantArgs a, hipStream_t st) {
    begin_launches();
    const dim3 grid(mx_rows_grid(a.nvec)), block(MX_TPB);
    if (fmt == FQ_MX_FP4_E2M1) launch(mx_dequant_kernel<DT, MXD_FP4, false, MX_VPT>, grid, block, st, a);
    else if (fmt == FQ_MX_FP8_E4M3) launch(mx_dequant_kernel<DT, MXD_FP8, false, MX_VPT>, grid, block, st, a);
    else launch(mx_dequant_kernel<DT, MXD_FP8, true, MX_VPT>, grid, block, st, a);
    return launch_result();
}

#define FQ_INSTANTIATE_MX_DEQUANT(DT) template int launch_mx_dequant<DT>(int, MxDequantArgs, hipStream_t);

}  // namespace fq
