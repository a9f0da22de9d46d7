// fq_mx_sr.h -- MX block-scaled fake quantization with STOCHASTIC rounding onto the element grid: the rounding rule
// for a gradient, whose backward GEMMs sum thousands of quantized elements -- under nearest rounding every element below half a quantum
// rounds to zero on every step (a bias); here E[y] = v.
//
//   mx_sr_kernel        the row axis: mx_kernel<DT, MX_FWD, ...>'s slots, load_clamped and mx_vec_absmax + DPP absmax (fq_mx.h)
//   mx_sr_cols_kernel   the column axis: the tile of fq_mx_cols.h through its stages mx_cols_load and mx_cols_consts; its own part is
//                       the constants of all four dwords up front and the row-outer loop (one Philox call per row of the strip)
// Both round through mx_rint_sr and mx_sr_dword below.  No rotation, no saturation bitmap, no export; no LDS, no barrier.
//
// Per block nothing changes up to the shared exponent (amax from the bit patterns, NaN / Inf -> a NaN block, E by the floor or ceil rule,
// t = v * 2^-E, the binade sb of |t| clamped at the smallest normal one).  a = |t| / quantum is the exact fp32 value mx_rint feeds to
// rintf; here
//     n = floor(a), f = a - n (both exact), up = float(R16) < f * 65536 (both sides exact), r = n + up
// and r goes through mx_value as before (a carry lands on the next binade's grid, saturation at max-normal, the input's sign, one rounding
// to the dtype).  P(up) = ceil(f * 2^16) / 2^16: exactly unbiased whenever f has at most 16 fractional bits, a bias below 2^-16 quantum
// otherwise.  Under CEIL nothing saturates, so E[y] = v for the whole block; under the floor rule the top binade still clips.
//
// R16 of flat element i (row-major in the contiguous tensor; both kernels: i = r * cols + c) is 16 bits of Philox4x32-10 on
//     key = (seed lo, seed hi), counter = (c lo, c hi, stream lo, stream hi), c = i >> 3;  j = i & 7: R16 = (word[j >> 1] >> 16 * (j & 1)) & 0xFFFF
// so one call serves 8 consecutive elements: one 16-byte vector of a 16-bit tensor, two of an fp32 one.  Both tensors are whole vectors
// per row, so flat vector w (as both kernels already index their loads) holds the elements w * EPV ..: the 16-bit lane makes one call per
// vector and uses all four words; the fp32 lane makes the call of its vector's pair and uses words 2 * (w & 1), 2 * (w & 1) + 1 -- the
// call is computed twice, once in each lane of the pair (DESIGN.md section 19 says why not exchanged).
#pragma once
#include "fq_mx_cols.h"

namespace fq {

// Philox4x32-10 (Salmon et al., SC'11; the generator PyTorch uses on devices): c <- 10 rounds of
//   hi0:lo0 = M0 * c0, hi1:lo1 = M1 * c2, c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), then the key bumped by (W0, W1)
__host__ __device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0, c[1] = (uint32_t)p1, c[2] = n2, c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
}

// the EPV / 2 words that hold the R16 of the EPV elements of flat vector w: element e of the vector takes (rw[e >> 1] >> 16 * (e & 1)) & 0xFFFF
template <int EPV> __host__ __device__ __forceinline__ void mx_sr_words(int64_t w, const MxSrKey& k, uint32_t (&rw)[EPV / 2]) {
    static_assert(EPV == 8 || EPV == 4, "a 16-byte vector of a 16-bit or a 32-bit type");
    const uint64_t cnt = EPV == 8 ? (uint64_t)w : (uint64_t)w >> 1;      // (w * EPV) >> 3
    uint32_t c[4] = {(uint32_t)cnt, (uint32_t)(cnt >> 32), k.s0, k.s1};
    philox4x32_10(c, k.k0, k.k1);
    if constexpr (EPV == 8) {
        rw[0] = c[0], rw[1] = c[1], rw[2] = c[2], rw[3] = c[3];
    } else {
        const bool odd = (w & 1) != 0;
        rw[0] = odd ? c[2] : c[0], rw[1] = odd ? c[3] : c[1];
    }
}

// mx_rint with the stochastic rule: r16 is the element's random number in [0, 65535]; -> r >= 0 (mx_value takes the sign from v)
__device__ __forceinline__ float mx_rint_sr(float v, int nE, int bmin, int mbits, uint32_t r16, int& sb) {
    const float a = __builtin_fabsf(mx_quanta(v, nE, bmin, mbits, sb));
    const float n = __builtin_floorf(a), f = a - n;
    return n + ((float)r16 < f * 65536.0f ? 1.0f : 0.0f);   // (a select and an add: `? n + 1 : n` compiles to a branch per element)
}

// the EPD elements of dword `word` (dword d of a vector) -> fake-quantized and packed; rw: mx_sr_words of the vector
template <int DT> __device__ __forceinline__ uint32_t mx_sr_dword(uint32_t word, int d, const uint32_t* rw, const int* nE, const int* yk, const float* maxx,
                                                                  const bool* bad, int bmin, int mbits) {
    using T = Ty<DT>;
    float fd[T::EPD];
    T::unpack(word, fd);
#pragma unroll
    for (int k = 0; k < T::EPD; ++k) {
        const int e = d * T::EPD + k;                                      // element of the vector
        const uint32_t r16 = (e & 1) ? rw[e >> 1] >> 16 : rw[e >> 1] & 0xFFFFu;
        int sb;
        const float rr = mx_rint_sr(fd[k], nE[k], bmin, mbits, r16, sb);
        float y = mx_value(fd[k], rr, sb, yk[k], maxx[k]);
        asm("" : "+v"(y));   // the value is computed for every lane and selected: without this the chain is sunk into a branch per element
        fd[k] = bad[k] ? as_f(0x7FC00000u) : y;
    }
    return T::pack(fd);
}

template <int DT, int VPT, bool CEIL>
__global__ __launch_bounds__(MX_TPB) void mx_sr_kernel(MxArgs a, MxFmt f, MxSrKey key) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE;     // elements per vector
    constexpr int BV = 32 / EPV;           // vectors per block
    const int64_t base = (int64_t)blockIdx.x * (MX_TPB * VPT) + threadIdx.x;
    const uint4* __restrict__ xv = (const uint4*)a.x;

    // out-of-range slots re-load the last vector and are never stored, as in mx_kernel
    uint4 r[VPT];
    if (a.ntl) load_clamped<true, VPT, MX_TPB>(r, xv, base, a.nvec);
    else load_clamped<false, VPT, MX_TPB>(r, xv, base, a.nvec);

    const int bmin = f.emin + 127;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int64_t v = base + i * MX_TPB;
        const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
        const uint32_t ab = group_reduce<OpMaxU>(mx_vec_absmax<DT>(r[i]), BV);   // fp32 bits of the block's amax (NaN sorts above Inf)
        bool bad[T::EPD];
        int nE[T::EPD], yk[T::EPD];
        float maxx[T::EPD];
        // mx_block_consts' text, not a call of it: through the helper the two fp32 instantiations come out three s_nop longer, and no
        // recorded benchmark launches them to show that this costs nothing
        const int E = CEIL ? mx_shared_exp_ceil(ab, f.emax, f.maxnorm) : mx_shared_exp(ab, f.emax);
#pragma unroll
        for (int k = 0; k < T::EPD; ++k) {                    // one block per vector: the same constants for both halves of a dword
            bad[k] = ab >= 0x7F800000u;
            nE[k] = -E, yk[k] = E - 127 - f.mbits;
            maxx[k] = __builtin_amdgcn_ldexpf(f.maxnorm, E);
        }
        uint32_t rw[EPV / 2];
        mx_sr_words<EPV>(v, key, rw);
        uint32_t o[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = mx_sr_dword<DT>(w[d], d, rw, nE, yk, maxx, bad, bmin, f.mbits);
        if (v < a.nvec) st16<true>(&((uint4*)a.y)[v], make_uint4(o[0], o[1], o[2], o[3]));
    }
}

template <int DT, bool CEIL>
__global__ __launch_bounds__(MX_TPB) void mx_sr_cols_kernel(MxColsArgs a, MxFmt f, MxSrKey key) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE;
    constexpr int RPL = MXC_TILE_ROWS / MXC_ROW_GROUPS;   // rows per lane
    uint32_t w[RPL][4], acc[4];
    bool live;
    const int64_t first = mx_cols_load<DT, RPL>(a, w, acc, live);

    const int bmin = f.emin + 127;
    bool bad[4][T::EPD];
    int nE[4][T::EPD], yk[4][T::EPD];
    float maxx[4][T::EPD];
#pragma unroll
    for (int d = 0; d < 4; ++d) mx_cols_consts<DT, CEIL>(acc[d], f, bad[d], nE[d], yk[d], maxx[d]);
#pragma unroll
    for (int i = 0; i < RPL; ++i) {                         // one row of the strip = one flat vector = one call's words
        const int64_t v = first + i * a.ncs;               // one value for the counter and the store's address (spelled twice: + 2 VGPRs)
        uint32_t rw[EPV / 2];
        mx_sr_words<EPV>(v, key, rw);
        uint32_t o[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) o[d] = mx_sr_dword<DT>(w[i][d], d, rw, nE[d], yk[d], maxx[d], bad[d], bmin, f.mbits);
        if (live) st16<true>(&((uint4*)a.y)[v], make_uint4(o[0], o[1], o[2], o[3]));
    }
}

// a and f validated by fqs_mx_fwd (fq_api.hip): nvec > 0, grid within limits
template <int DT> int launch_mx_sr(bool ceil, MxArgs a, MxFmt f, MxSrKey k, hipStream_t st) {
    begin_launches();
    const dim3 grid(mx_rows_grid(a.nvec));
    if (ceil) launch(mx_sr_kernel<DT, MX_VPT, true>, grid, dim3(MX_TPB), st, a, f, k);
    else launch(mx_sr_kernel<DT, MX_VPT, false>, grid, dim3(MX_TPB), st, a, f, k);
    return launch_result();
}

// a and f validated by fqs_mx_fwd_cols (fq_api.hip): whole 32-row tiles, ncs > 0, row_tiles * a.nct within one launch's grid
template <int DT> int launch_mx_sr_cols(bool ceil, MxColsArgs a, MxFmt f, MxSrKey k, int64_t row_tiles, hipStream_t st) {
    begin_launches();
    const dim3 grid((unsigned)(row_tiles * a.nct));
    if (ceil) launch(mx_sr_cols_kernel<DT, true>, grid, dim3(MX_TPB), st, a, f, k);
    else launch(mx_sr_cols_kernel<DT, false>, grid, dim3(MX_TPB), st, a, f, k);
    return launch_result();
}

#define FQ_INSTANTIATE_MX_SR(DT)                                                      \
    template int launch_mx_sr<DT>(bool, MxArgs, MxFmt, MxSrKey, hipStream_t);         \
    template int launch_mx_sr_cols<DT>(bool, MxColsArgs, MxFmt, MxSrKey, int64_t, hipStream_t);

}  // namespace fq
