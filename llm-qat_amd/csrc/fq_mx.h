// fq_mx.h -- OCP Microscaling (MX) block-scaled fake quantization: every 32 consecutive elements of the last dimension share one
// power-of-two (E8M0) scale, and each element is rounded onto a narrow float grid (FP4 E2M1, FP6 E2M3 / E3M2, FP8 E4M3 / E5M2).
//
//   mx_kernel           a contiguous tensor whose last dimension is a multiple of 32 is a flat sequence of independent blocks: no
//                       rows, no row bounds, no mask, no LDS.  Lane t of workgroup b owns the 16-byte vectors b * TPB * VPT + i * TPB + t
//                       (VPT of them in flight).  A block is BV = 32 * esize / 16 consecutive vectors (4 for bf16 / fp16, 8 for fp32),
//                       so it lies in an aligned BV-lane segment and its absmax is a DPP reduction over that segment (group_reduce).
//                       KIND = MX_FWD writes the fake-quantized tensor; MX_EXP4 / MX_EXP8 write packed element codes (two per byte,
//                       element 2k in the low nibble of byte k / one OCP byte per element) and one E8M0 byte per block.
//
// Semantics (per block, fp32 arithmetic):
//   amax = max|v|; a NaN / Inf in the block makes every output NaN (export: scale 0xFF, codes 0).
//   E = clamp(floor(log2 amax) - emax, -127, 127) (amax == 0: E = -127); t = v * 2^-E (exact); q = t rounded to nearest-even onto the
//   element grid (normals and subnormals), saturated to +-max-normal, sign kept; y = q * 2^E (exact in fp32), rounded once to the dtype.
// The format is a kernel argument (MxFmt): the rounding chain is the same for all five, so only the dtype and the output kind are
// template parameters.
#pragma once
#include "fq_group.h"

namespace fq {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// E of a finite block from the fp32 bits of its amax, read from the bits (a subnormal amax included)
__device__ __forceinline__ int mx_shared_exp(uint32_t ab, int emax) {
    const int f = (int)(ab >> 23);
    int e = f ? f - 127 : 31 - (int)__builtin_clz(ab | 1u) - 149;
    e = ab ? e - emax : -127;
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// one element of a finite block, step 1: t = v * 2^-E (nE = -E; exact: t only underflows far below the grid) in units of its quantum,
// rounded to nearest-even (v_rndne_f32).  bmin = emin + 127, the biased exponent of the smallest normal binade; sb <- the biased exponent
// of t's binade, at least bmin (the subnormals share the smallest normal binade's quantum).
__device__ __forceinline__ float mx_rint(float v, int nE, int bmin, int mbits, int& sb) {
    const float t = __builtin_amdgcn_ldexpf(v, nE);
    const int e = (int)((as_u(t) >> 23) & 0xFFu);                          // 0 for a subnormal t
    sb = e > bmin ? e : bmin;
    return __builtin_rintf(__builtin_amdgcn_ldexpf(t, 127 + mbits - sb));
}

// step 2 (forward): y = q * 2^E from r (yk = E - 127 - mbits), saturated at maxx = max-normal * 2^E (exact), with the input's sign
__device__ __forceinline__ float mx_value(float v, float r, int sb, int yk, float maxx) {
    const float q = __builtin_fminf(__builtin_fabsf(__builtin_amdgcn_ldexpf(r, sb + yk)), maxx);
    return __builtin_copysignf(q, v);
}

// code of one element: ((binade - smallest normal binade) << mbits) + |r| is the OCP encoding of |q| (a carry of r into the next
// binade lands on that binade's code), min with the largest normal's code saturates, the sign bit is the input's
__device__ __forceinline__ uint32_t mx_code(float v, float r, int sb_rel, const MxFmt& f) {
    uint32_t c = ((uint32_t)sb_rel << f.mbits) + (uint32_t)__builtin_fabsf(r);
    c = c < f.maxcode ? c : f.maxcode;
    return (as_u(v) >> 31) ? c | f.signbit : c;
}

template <int DT, int KIND, int VPT>
__global__ __launch_bounds__(MX_TPB) void mx_kernel(MxArgs a, MxFmt f) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE;     // elements per vector
    constexpr int BV = 32 / EPV;           // vectors per block
    const int64_t base = (int64_t)blockIdx.x * (MX_TPB * VPT) + threadIdx.x;
    const uint4* __restrict__ xv = (const uint4*)a.x;

    // Out-of-range slots re-load the last vector: nvec is a multiple of BV and segments are BV-aligned, so such a slot's whole block
    // is out of range and is never stored.
    uint4 r[VPT];
    if (a.ntl) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int64_t v = base + i * MX_TPB;
            r[i] = ld16<true>(&xv[v < a.nvec ? v : a.nvec - 1]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int64_t v = base + i * MX_TPB;
            r[i] = ld16<false>(&xv[v < a.nvec ? v : a.nvec - 1]);
        }
    }

    const int bmin = f.emin + 127;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t v = base + i * MX_TPB;
        uint32_t acc = 0;
        acc = T::absmax_acc(acc, r[i].x);
        acc = T::absmax_acc(acc, r[i].y);
        acc = T::absmax_acc(acc, r[i].z);
        acc = T::absmax_acc(acc, r[i].w);
        const uint32_t ab = group_reduce<OpMaxU>(T::absmax_finish(acc), BV);   // fp32 bits of the block's amax (NaN sorts above Inf)
        const bool bad = ab >= 0x7F800000u;                                     // a NaN or Inf in the block
        const int E = mx_shared_exp(ab, f.emax);
        const int nE = -E, yk = E - 127 - f.mbits;
        const float maxx = __builtin_amdgcn_ldexpf(f.maxnorm, E);
        const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
        if constexpr (KIND == MX_FWD) {
            uint32_t o[4];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float fd[T::EPD];
                T::unpack(w[d], fd);
#pragma unroll
                for (int k = 0; k < T::EPD; ++k) {
                    int sb;
                    const float rr = mx_rint(fd[k], nE, bmin, f.mbits, sb);
                    fd[k] = bad ? as_f(0x7FC00000u) : mx_value(fd[k], rr, sb, yk, maxx);
                }
                o[d] = T::pack(fd);
            }
            if (v < a.nvec) st16<true>(&((uint4*)a.y)[v], make_uint4(o[0], o[1], o[2], o[3]));
        } else {
            uint32_t c[EPV];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float fd[T::EPD];
                T::unpack(w[d], fd);
#pragma unroll
                for (int k = 0; k < T::EPD; ++k) {
                    int sb;
                    const float rr = mx_rint(fd[k], nE, bmin, f.mbits, sb);
                    const uint32_t code = mx_code(fd[k], rr, sb - bmin, f);
                    c[d * T::EPD + k] = bad ? 0u : code;
                }
            }
            if (v < a.nvec) {
                if constexpr (KIND == MX_EXP8) {   // one byte per element: EPV bytes per vector
                    uint32_t b[EPV / 4];
#pragma unroll
                    for (int j = 0; j < EPV / 4; ++j) b[j] = c[4 * j] | (c[4 * j + 1] << 8) | (c[4 * j + 2] << 16) | (c[4 * j + 3] << 24);
                    if constexpr (EPV == 8) {
                        const u32x2_t b2 = {b[0], b[1]};
                        __builtin_nontemporal_store(b2, (u32x2_t*)(a.elems + v * 8));
                    } else {
                        __builtin_nontemporal_store(b[0], (uint32_t*)(a.elems + v * 4));
                    }
                } else {                            // two codes per byte, element 2k in the low nibble of byte k
                    uint32_t b = 0;
#pragma unroll
                    for (int j = 0; j < EPV; ++j) b |= c[j] << (4 * j);
                    if constexpr (EPV == 8) __builtin_nontemporal_store(b, (uint32_t*)(a.elems + v * 4));
                    else __builtin_nontemporal_store((uint16_t)b, (uint16_t*)(a.elems + v * 2));
                }
                if ((threadIdx.x & (BV - 1)) == 0) a.scales[v / BV] = bad ? (uint8_t)0xFF : (uint8_t)(E + 127);
            }
        }
    }
}

template <int DT, int KIND> static void launch_mx_kind(const MxArgs& a, const MxFmt& f, hipStream_t st) {
    const int64_t grid = (a.nvec + MX_TPB * MX_VPT - 1) / (MX_TPB * MX_VPT);
    FQ_LAUNCHK((mx_kernel<DT, KIND, MX_VPT>), dim3((unsigned)grid), dim3(MX_TPB), 0, st, a, f);
}

// kind: MX_FWD / MX_EXP4 / MX_EXP8; a and f validated by fq_mx_fwd / fq_mx_export (nvec > 0, grid within limits)
template <int DT> int launch_mx(int kind, MxArgs a, MxFmt f, hipStream_t st) {
    begin_launches();
    if (kind == MX_FWD) launch_mx_kind<DT, MX_FWD>(a, f, st);
    else if (kind == MX_EXP4) launch_mx_kind<DT, MX_EXP4>(a, f, st);
    else launch_mx_kind<DT, MX_EXP8>(a, f, st);
    return launch_result();
}

#define FQ_INSTANTIATE_MX(DT) template int launch_mx<DT>(int, MxArgs, MxFmt, hipStream_t);

}  // namespace fq
