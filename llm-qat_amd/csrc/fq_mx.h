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
// The format is a kernel argument (MxFmt): the rounding chain is the same for all five, so only the dtype, the output kind and the
// rotation are template parameters.
//
// Scale rule and saturation mask.  CEIL picks the no-clip rule: E is one higher where amax * 2^-E would exceed
// max-normal, so no element of a finite block saturates.  It is a template parameter: as a kernel argument it cost the existing entry
// points 1 - 2 % on a bf16 [4096, 11008] tensor, several times their run-to-run scatter, and with CEIL = false and MASK = false the kernels
// are the ones that were there before.  MASK (MX_FWD only) also writes one bit per element, 0 where the rounded value on the unbounded grid exceeds
// max-normal (saturation changed it): a lane's EPV bits go to their place in the block's 32-bit word, the word is an OR over the block's BV
// lanes (group_reduce) and one lane stores it.  Under ROT the bits are those of the elements of x R.
//   mx_ste_kernel       the masked straight-through backward: gx = g where the bit is 1, else +0.0, a select on bit patterns; ROT: the
//                       masked gradient goes through mx_rotate and is rounded once, as KIND = MX_ROT does (one launch).
//
// ROT: the kernel quantizes x R instead of x.  R is block-diagonal along the last dimension with blocks H64 / 8
// (H64 the 64 x 64 Sylvester Hadamard matrix): orthonormal, symmetric, its own inverse, entries +-0.125.  A run of 64 elements is 8
// consecutive vectors of a 16-bit tensor (16 of an fp32 one), held by 8 (16) lanes of one DPP row.  The run is widened to fp32, the
// butterfly stages 1, 2, 4, .. 32 on the element index run in that order -- the strides below a vector in the lane's registers, the others
// as lane exchanges -- and the result is multiplied by 0.125f; the MX chain then runs on these fp32 values (amax from fp32 bits, sign from
// the rotated value, a sum that overflows makes a NaN block).  No LDS, no barrier.  KIND = MX_ROT rounds x R once to the dtype.
// The exchanges need the lane that holds vector w ^ 1, w ^ 2, w ^ 4 (w ^ 8), and DPP has lane ^ 1, lane ^ 2 (quad_perm), lane ^ 7
// (row_half_mirror) and lane ^ 15 (row_mirror) but no lane ^ 4 or lane ^ 8.  So lane l of a run holds vector w = mx_rot_slot(l), chosen so
// that the mirrors flip exactly one bit of w; the run's lanes still cover the same aligned 128 (256) bytes.
#pragma once
#include "fq_group.h"

namespace fq {

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

struct OpOrU {   // idempotent, so group_reduce's butterfly serves it
    __device__ static __forceinline__ uint32_t f(uint32_t a, uint32_t b) { return a | b; }
};

// E of a finite block from the fp32 bits of its amax, read from the bits (a subnormal amax included)
__device__ __forceinline__ int mx_shared_exp(uint32_t ab, int emax) {
    const int f = (int)(ab >> 23);
    int e = f ? f - 127 : 31 - (int)__builtin_clz(ab | 1u) - 149;
    e = ab ? e - emax : -127;
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}
// the ceil rule: amax * 2^-Ef (exact, in [2^emax, 2^(emax + 1))) above max-normal takes Ef + 1, before the clamp
__device__ __forceinline__ int mx_shared_exp_ceil(uint32_t ab, int emax, float maxnorm) {
    const int f = (int)(ab >> 23);
    int e = (f ? f - 127 : 31 - (int)__builtin_clz(ab | 1u) - 149) - emax;
    e += (int)(__builtin_amdgcn_ldexpf(as_f(ab), -e) > maxnorm);
    e = ab ? e : -127;
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// what the element chain needs of a block, from the fp32 bits of its amax (NaN sorts above Inf): bad = a NaN or Inf in the block,
// nE = -E, yk = E - 127 - mbits, maxx = max-normal * 2^E (exact)
template <bool CEIL> __device__ __forceinline__ void mx_block_consts(uint32_t ab, const MxFmt& f, bool& bad, int& nE, int& yk, float& maxx) {
    bad = ab >= 0x7F800000u;
    const int E = CEIL ? mx_shared_exp_ceil(ab, f.emax, f.maxnorm) : mx_shared_exp(ab, f.emax);
    nE = -E, yk = E - 127 - f.mbits;
    maxx = __builtin_amdgcn_ldexpf(f.maxnorm, E);
}

// one element of a finite block, step 1, shared by both rounding rules: -> t = v * 2^-E (nE = -E; exact: t only underflows far below
// the grid) in units of its quantum.  bmin = emin + 127, the biased exponent of the smallest normal binade; sb <- the biased exponent of
// t's binade, at least bmin (the subnormals share the smallest normal binade's quantum).
__device__ __forceinline__ float mx_quanta(float v, int nE, int bmin, int mbits, int& sb) {
    const float t = __builtin_amdgcn_ldexpf(v, nE);
    const int e = (int)((as_u(t) >> 23) & 0xFFu);                          // 0 for a subnormal t
    sb = e > bmin ? e : bmin;
    return __builtin_amdgcn_ldexpf(t, 127 + mbits - sb);
}
// ... rounded to nearest-even (v_rndne_f32); the stochastic rule is mx_rint_sr (fq_mx_sr.h)
__device__ __forceinline__ float mx_rint(float v, int nE, int bmin, int mbits, int& sb) { return __builtin_rintf(mx_quanta(v, nE, bmin, mbits, sb)); }

// step 2 (forward): y = q * 2^E from r (yk = E - 127 - mbits), saturated at maxx = max-normal * 2^E (exact), with the input's sign
__device__ __forceinline__ float mx_value(float v, float r, int sb, int yk, float maxx) {
    const float q = __builtin_fminf(__builtin_fabsf(__builtin_amdgcn_ldexpf(r, sb + yk)), maxx);
    return __builtin_copysignf(q, v);
}
// the same, and sat <- whether the saturation changed the value (the rounded magnitude, before the min, is above maxx)
__device__ __forceinline__ float mx_value_sat(float v, float r, int sb, int yk, float maxx, bool& sat) {
    const float u = __builtin_fabsf(__builtin_amdgcn_ldexpf(r, sb + yk));
    sat = u > maxx;
    return __builtin_copysignf(__builtin_fminf(u, maxx), v);
}

// code of one element: ((binade - smallest normal binade) << mbits) + |r| is the OCP encoding of |q| (a carry of r into the next
// binade lands on that binade's code), min with the largest normal's code saturates, the sign bit is the input's
__device__ __forceinline__ uint32_t mx_code(float v, float r, int sb_rel, const MxFmt& f) {
    uint32_t c = ((uint32_t)sb_rel << f.mbits) + (uint32_t)__builtin_fabsf(r);
    c = c < f.maxcode ? c : f.maxcode;
    return (as_u(v) >> 31) ? c | f.signbit : c;
}

// vector (within the workgroup's slot) of lane t under ROT: bit 2 of w is t's, bits 0 and 1 are t's xor bit 2 -> t ^ 7 is w ^ 4 and
// t ^ 1, t ^ 2 are w ^ 1, w ^ 2; fp32 (16 lanes per run): bit 3 is t's and bit 2 is xored with it -> t ^ 15 is w ^ 8, t ^ 7 still w ^ 4
template <int EPV> __device__ __forceinline__ uint32_t mx_rot_slot(uint32_t t) {
    uint32_t w = t ^ (((t >> 2) & 1u) * 3u);
    if constexpr (EPV == 4) w ^= ((t >> 3) & 1u) * 4u;
    return w;
}

// one exchange stage: the lane whose vector has the stage's bit clear takes v + partner, the other partner - v = partner + (-v), so both
// are one IEEE add of the partner's value (DPP) and the lane's own value with its sign flipped by sgn (0 or 0x80000000)
template <int CTRL, int EPV> __device__ __forceinline__ void mx_rot_exchange(float (&v)[EPV], uint32_t sgn) {
#pragma unroll
    for (int e = 0; e < EPV; ++e) v[e] = as_f(dpp<CTRL>(as_u(v[e]))) + as_f(as_u(v[e]) ^ sgn);
}

// v: the lane's EPV consecutive elements of a run, w: the lane's vector index (only its low bits matter) -> the lane's elements of
// (run) H64 * 0.125, every add / subtract one fp32 operation, stages in the order of the definition
template <int EPV> __device__ __forceinline__ void mx_rotate(float (&v)[EPV], uint32_t w) {
#pragma unroll
    for (int s = 1; s < EPV; s *= 2) {
#pragma unroll
        for (int j = 0; j < EPV; ++j) {
            if (!(j & s)) {
                const float p = v[j], q = v[j + s];
                v[j] = p + q;
                v[j + s] = p - q;
            }
        }
    }
    mx_rot_exchange<0xB1, EPV>(v, (w & 1u) << 31);            // quad_perm:[1,0,3,2]: w ^ 1
    mx_rot_exchange<0x4E, EPV>(v, (w & 2u) << 30);            // quad_perm:[2,3,0,1]: w ^ 2
    mx_rot_exchange<0x141, EPV>(v, (w & 4u) << 29);           // row_half_mirror:     w ^ 4
    if constexpr (EPV == 4) mx_rot_exchange<0x140, EPV>(v, (w & 8u) << 28);   // row_mirror: w ^ 8
#pragma unroll
    for (int e = 0; e < EPV; ++e) v[e] = v[e] * 0.125f;
}

// fp32 bits of max|x| over the elements of one loaded vector
template <int DT> __device__ __forceinline__ uint32_t mx_vec_absmax(const uint4& r) {
    using T = Ty<DT>;
    return T::absmax_finish(T::absmax_acc(T::absmax_acc(T::absmax_acc(T::absmax_acc(0u, r.x), r.y), r.z), r.w));
}

// workgroups of a launch of the row kernels: MX_VPT vectors per lane
inline unsigned mx_rows_grid(int64_t nvec) { return (unsigned)((nvec + MX_TPB * MX_VPT - 1) / (MX_TPB * MX_VPT)); }

template <int DT, int KIND, int VPT, bool ROT, bool MASK, bool CEIL>
__global__ __launch_bounds__(MX_TPB) void mx_kernel(MxArgs a, MxFmt f) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE;     // elements per vector
    constexpr int BV = 32 / EPV;           // vectors per block
    static_assert(ROT || KIND != MX_ROT, "the rotation alone is a rotated launch");
    static_assert(!MASK || KIND == MX_FWD, "the saturation bitmap belongs to the forward");
    const uint32_t slot = ROT ? mx_rot_slot<EPV>(threadIdx.x) : threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (MX_TPB * VPT) + slot;
    const uint4* __restrict__ xv = (const uint4*)a.x;

    // Out-of-range slots re-load the last vector: nvec is a multiple of BV and segments are BV-aligned, so such a slot's whole block
    // is out of range and is never stored.  (ROT: nvec is a multiple of the run's vector count and runs are aligned, likewise.)
    uint4 r[VPT];
    if (a.ntl) load_clamped<true, VPT, MX_TPB>(r, xv, base, a.nvec);
    else load_clamped<false, VPT, MX_TPB>(r, xv, base, a.nvec);

    const int bmin = f.emin + 127;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t v = base + i * MX_TPB;
        const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
        float xr[ROT ? EPV : 1];   // ROT: the lane's elements of x R
        uint32_t acc = 0;
        if constexpr (ROT) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float fd[T::EPD];
                T::unpack(w[d], fd);
#pragma unroll
                for (int k = 0; k < T::EPD; ++k) xr[d * T::EPD + k] = fd[k];
            }
            mx_rotate<EPV>(xr, slot);
            if constexpr (KIND == MX_ROT) {
                uint32_t o[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    float fd[T::EPD];
#pragma unroll
                    for (int k = 0; k < T::EPD; ++k) fd[k] = xr[d * T::EPD + k];
                    o[d] = T::pack(fd);
                }
                if (v < a.nvec) st16<true>(&((uint4*)a.y)[v], make_uint4(o[0], o[1], o[2], o[3]));
                continue;
            }
#pragma unroll
            for (int e = 0; e < EPV; ++e) acc = Ty<F32>::absmax_acc(acc, as_u(xr[e]));
        } else {
            acc = mx_vec_absmax<DT>(r[i]);
        }
        bool bad;
        int nE, yk;
        float maxx;
        mx_block_consts<CEIL>(group_reduce<OpMaxU>(acc, BV), f, bad, nE, yk, maxx);   // the block's amax: a DPP max over its BV lanes
        if constexpr (KIND == MX_FWD) {
            uint32_t o[4];
            uint32_t keep = 0;   // MASK: bit e set = the lane's element e was not changed by the saturation
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float fd[T::EPD];
                if constexpr (ROT) {
#pragma unroll
                    for (int k = 0; k < T::EPD; ++k) fd[k] = xr[d * T::EPD + k];
                } else {
                    T::unpack(w[d], fd);
                }
#pragma unroll
                for (int k = 0; k < T::EPD; ++k) {
                    int sb;
                    const float rr = mx_rint(fd[k], nE, bmin, f.mbits, sb);
                    if constexpr (MASK) {
                        bool sat;
                        const float yv = mx_value_sat(fd[k], rr, sb, yk, maxx, sat);
                        fd[k] = bad ? as_f(0x7FC00000u) : yv;
                        keep |= (uint32_t)(bad || !sat) << (d * T::EPD + k);
                    } else {
                        fd[k] = bad ? as_f(0x7FC00000u) : mx_value(fd[k], rr, sb, yk, maxx);
                    }
                }
                o[d] = T::pack(fd);
            }
            if (v < a.nvec) st16<true>(&((uint4*)a.y)[v], make_uint4(o[0], o[1], o[2], o[3]));
            if constexpr (MASK) {   // flat element i is bit i & 31 of word i >> 5: vector v holds the bits (v % BV) * EPV .. of word v / BV
                const uint32_t word = group_reduce<OpOrU>(keep << ((uint32_t)(v & (BV - 1)) * EPV), BV);
                if (v < a.nvec && (threadIdx.x & (BV - 1)) == 0) ((uint32_t*)a.elems)[v / BV] = word;
            }
        } else {
            uint32_t c[EPV];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float fd[T::EPD];
                if constexpr (ROT) {
#pragma unroll
                    for (int k = 0; k < T::EPD; ++k) fd[k] = xr[d * T::EPD + k];
                } else {
                    T::unpack(w[d], fd);
                }
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
                if ((threadIdx.x & (BV - 1)) == 0) a.scales[v / BV] = bad ? (uint8_t)0xFF : (uint8_t)(127 - nE);
            }
        }
    }
}

// mx_ste_kernel's loads: the lane's VPT vectors of g, clamped as load_clamped clamps, and in the low bits of m[i] the EPV mask bits of
// vector i -- bits (v % BV) * EPV .. of mask word v / BV
template <bool NT, int DT, int VPT> __device__ __forceinline__ void mx_ste_load(const MxSteArgs& a, int64_t base, uint4 (&r)[VPT], uint32_t (&m)[VPT]) {
    constexpr int EPV = 16 / Ty<DT>::ESIZE, BV = 32 / EPV;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t v = base + i * MX_TPB, c = v < a.nvec ? v : a.nvec - 1;
        r[i] = ld16<NT>(&((const uint4*)a.g)[c]);
        m[i] = a.mask[c / BV] >> ((uint32_t)(c & (BV - 1)) * EPV);
    }
}

// gx = g where the mask bit is 1, else +0.0 (a select on the bit patterns: a NaN g at a masked position gives +0.0); ROT: the masked
// values times R, rounded once.  Slots and stores as mx_kernel.
template <int DT, int VPT, bool ROT>
__global__ __launch_bounds__(MX_TPB) void mx_ste_kernel(MxSteArgs a) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE;
    const uint32_t slot = ROT ? mx_rot_slot<EPV>(threadIdx.x) : threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (MX_TPB * VPT) + slot;

    uint4 r[VPT];
    uint32_t m[VPT];
    if (a.ntl) mx_ste_load<true, DT>(a, base, r, m);
    else mx_ste_load<false, DT>(a, base, r, m);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t v = base + i * MX_TPB;
        uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            uint32_t keep = 0;
#pragma unroll
            for (int k = 0; k < T::EPD; ++k)
                if ((m[i] >> (d * T::EPD + k)) & 1u) keep |= (T::EPD == 1 ? 0xFFFFFFFFu : 0xFFFFu << (16 * k));
            w[d] &= keep;
        }
        if constexpr (ROT) {
            float xr[EPV];
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float fd[T::EPD];
                T::unpack(w[d], fd);
#pragma unroll
                for (int k = 0; k < T::EPD; ++k) xr[d * T::EPD + k] = fd[k];
            }
            mx_rotate<EPV>(xr, slot);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                float fd[T::EPD];
#pragma unroll
                for (int k = 0; k < T::EPD; ++k) fd[k] = xr[d * T::EPD + k];
                w[d] = T::pack(fd);
            }
        }
        if (v < a.nvec) st16<true>(&((uint4*)a.gx)[v], make_uint4(w[0], w[1], w[2], w[3]));
    }
}

template <int DT, int KIND, bool ROT = false, bool MASK = false, bool CEIL = false>
static void launch_mx_kind(const MxArgs& a, const MxFmt& f, hipStream_t st) {
    launch(mx_kernel<DT, KIND, MX_VPT, ROT, MASK, CEIL>, dim3(mx_rows_grid(a.nvec)), dim3(MX_TPB), st, a, f);
}
template <int DT, bool ROT, bool CEIL> static void launch_mx_rule(int kind, bool mask, const MxArgs& a, const MxFmt& f, hipStream_t st) {
    if (kind == MX_FWD && mask) launch_mx_kind<DT, MX_FWD, ROT, true, CEIL>(a, f, st);
    else if (kind == MX_FWD) launch_mx_kind<DT, MX_FWD, ROT, false, CEIL>(a, f, st);
    else if (kind == MX_EXP4) launch_mx_kind<DT, MX_EXP4, ROT, false, CEIL>(a, f, st);
    else launch_mx_kind<DT, MX_EXP8, ROT, false, CEIL>(a, f, st);
}
// a and f validated by mx_entry (fq_api.hip): nvec > 0, grid within limits, rot: whole rotation runs, mask only with MX_FWD, MX_ROT only
// with rot and without ceil / mask
template <int DT> int launch_mx(int kind, bool rot, bool ceil, bool mask, MxArgs a, MxFmt f, hipStream_t st) {
    begin_launches();
    if (kind == MX_ROT) launch_mx_kind<DT, MX_ROT, true>(a, f, st);
    else if (rot && ceil) launch_mx_rule<DT, true, true>(kind, mask, a, f, st);
    else if (rot) launch_mx_rule<DT, true, false>(kind, mask, a, f, st);
    else if (ceil) launch_mx_rule<DT, false, true>(kind, mask, a, f, st);
    else launch_mx_rule<DT, false, false>(kind, mask, a, f, st);
    return launch_result();
}

// a validated by fq_mx_ste_bwd (nvec > 0, grid within limits; rot: whole runs)
template <int DT> int launch_mx_ste(bool rot, MxSteArgs a, hipStream_t st) {
    begin_launches();
    const dim3 grid(mx_rows_grid(a.nvec));
    if (rot) launch(mx_ste_kernel<DT, MX_VPT, true>, grid, dim3(MX_TPB), st, a);
    else launch(mx_ste_kernel<DT, MX_VPT, false>, grid, dim3(MX_TPB), st, a);
    return launch_result();
}

#define FQ_INSTANTIATE_MX(DT)                                              \
    template int launch_mx<DT>(int, bool, bool, bool, MxArgs, MxFmt, hipStream_t); \
    template int launch_mx_ste<DT>(bool, MxSteArgs, hipStream_t);

}  // namespace fq
