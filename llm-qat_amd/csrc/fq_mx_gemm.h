// fq_mx_gemm.h -- block-scaled GEMM over MX exports on gfx950's scaled matrix instruction (v_mfma_scale_f32_16x16x128_f8f6f4):
//   out[m, n] = sum_k A[m, k] * W[n, k],   A an [M, K] export, W an [N, K] export (fq_mx_export's layout: K contiguous, one E8M0 byte
//   per 32 k), each independently FP4 E2M1 / FP8 E4M3 / FP8 E5M2; fp32 accumulation in the matrix core, one rounding to the output dtype.
//
// Operand layout (measured: tools/mx_mfma_probe.hip -> profiles/mx_mfma_layout.txt), lane l, g = l >> 4, of
// either operand (row l & 15 of the A operand / column l & 15 of the B operand), over one K step of 128:
//   fp4   the low 4 of the operand's 8 dwords: k = 32 g .. 32 g + 31, element j in nibble j, low nibble first -- 16 consecutive bytes
//         of an export row;
//   fp8   dwords 0..3: k = 16 g .. 16 g + 15, dwords 4..7: k = 64 + 16 g .. 64 + 16 g + 15, one byte each -- two runs of 16 consecutive
//         bytes of an export row, 64 bytes apart (NOT 32 consecutive k: that order passes fp8 x fp8 and fails against an fp4 operand);
//   scale the lane's byte scales k = 32 g .. 32 g + 31 of its row, whatever the format: byte 4 * step + g of the row's E8M0 bytes.
// So fragments load from global memory as whole 16-byte vectors with no shuffle, no LDS and no repacking.
// D: lane l, register i is row 4 * (l >> 4) + i, column l & 15.  W is the instruction's A operand (rows = n) and the activation its B
// operand (columns = m), so a lane ends with 4 consecutive n of one output row: one 16- / 8-byte store.
//
//   mx_gemm_tiled    128 (n) x 128 (m) per workgroup, 4 waves of 64 x 64 (4 x 4 instruction tiles, 64 accumulator registers); per K
//                    step of 128 a wave loads 4 + 4 fragments straight into registers, double-buffered over K (the loads of step s + 1
//                    are issued before the 16 MFMAs of step s).  Tail rows are clamped on load and masked on store.
//   mx_gemm_skinny   M <= 32 (decode): one workgroup per 16 rows of W, its 8 waves take the K steps round-robin, so W is read exactly
//                    once; the 8 partial tiles are summed through LDS in wave order (no atomics: run-to-run identical).
//
// NaN rule: the instruction itself returns NaN for every result whose row of A or column of B carries an 0xFF scale byte, zero elements
// included (measured by the probe), and NaN survives the accumulation over K and the skinny kernel's sum, so the kernels add nothing.
// Scale byte 0 is 2^-127 in the instruction as in MXExport.dequantize() (probe: 2^-127 x 2^127 x 128 = 128).
#pragma once
#include "fq_mx.h"

namespace fq {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// F: the instruction's format code of an operand (cbsz / blgp): 0 E4M3, 1 E5M2, 4 E2M1
template <int F> struct MxOperand {
    static constexpr int STEP_BYTES = F == 4 ? 64 : 128;      // 128 k of one row
    // p: the lane's first 16 bytes of the step (row start + step * STEP_BYTES + 16 * g; 16-byte aligned)
    static __device__ __forceinline__ i32x8_t load(const uint8_t* __restrict__ p) {
        const uint4 lo = *(const uint4*)p;
        if constexpr (F == 4) {
            return i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, 0, 0, 0, 0};
        } else {
            const uint4 hi = *(const uint4*)(p + 64);
            return i32x8_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
        }
    }
};

// the rows of one operand a lane reads: T instruction tiles of 16 rows, this lane's row of each (clamped to the tensor), its k block
template <int F, int T> struct MxRows {
    const uint8_t* e[T];   // row start + this lane's block offset within a K step
    const uint8_t* s[T];
    // row0: first row of the wave's tile; rows: rows of the tensor; K: elements per row
    __device__ __forceinline__ void init(const uint8_t* elems, const uint8_t* scales, int64_t row0, int64_t rows, int64_t K, int lane) {
        const int64_t ebytes = F == 4 ? K / 2 : K;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            int64_t r = row0 + 16 * t + (lane & 15);
            r = r < rows ? r : rows - 1;
            e[t] = elems + r * ebytes + (lane >> 4) * 16;
            s[t] = scales + r * (K / 32) + (lane >> 4);
        }
    }
};

template <int F, int T> struct MxFrags {
    i32x8_t v[T];
    int sc[T];
    __device__ __forceinline__ void load(const MxRows<F, T>& r, int64_t step) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            v[t] = MxOperand<F>::load(r.e[t] + step * MxOperand<F>::STEP_BYTES);
            sc[t] = r.s[t][step * 4];
        }
    }
};

// acc[tn][tm] += W tile tn x A tile tm over one K step
template <int FW, int FA, int TN, int TM>
__device__ __forceinline__ void mx_mma(f32x4_t (&acc)[TN][TM], const MxFrags<FW, TN>& w, const MxFrags<FA, TM>& a) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
            acc[tn][tm] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(w.v[tn], a.v[tm], acc[tn][tm], FW, FA, 0, w.sc[tn], 0, a.sc[tm]);
}

// dt: F32 / BF16 / F16 (the FQ_DTYPE_* codes), uniform over the launch
__device__ __forceinline__ void mx_store1(void* out, int64_t idx, float v, int dt) {
    if (dt == F32) Ty<F32>::store1(out, idx, v);
    else if (dt == BF16) Ty<BF16>::store1(out, idx, v);
    else Ty<F16>::store1(out, idx, v);
}

// out[m, n .. n + 3] <- v, masked at the tensor's edges; vec: N % 4 == 0 (n % 4 == 0 always: whole, aligned vectors, n + 3 < N)
__device__ __forceinline__ void mx_store4(void* out, int64_t m, int64_t n, int64_t M, int64_t N, f32x4_t v, int dt, bool vec) {
    if (m >= M || n >= N) return;
    const int64_t idx = m * N + n;
    if (vec) {
        if (dt == F32) {
            *(f32x4_t*)((float*)out + idx) = v;
        } else {
            const float lo[2] = {v[0], v[1]}, hi[2] = {v[2], v[3]};
            const u32x2_t o = dt == BF16 ? u32x2_t{Ty<BF16>::pack(lo), Ty<BF16>::pack(hi)} : u32x2_t{Ty<F16>::pack(lo), Ty<F16>::pack(hi)};
            *(u32x2_t*)((uint16_t*)out + idx) = o;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (n + i < N) mx_store1(out, idx + i, v[i], dt);
    }
}

constexpr int MXG_SKINNY_WAVES = 8;  // K split of the skinny kernel

template <int FW, int FA>
__global__ __launch_bounds__(256) void mx_gemm_tiled(MxGemmArgs g) {
    constexpr int TN = 4, TM = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t m0 = (int64_t)blockIdx.x * MXG_TILE + (wave & 1) * 64;
    const int64_t n0 = (int64_t)blockIdx.y * MXG_TILE + (wave >> 1) * 64;
    if (m0 >= g.M || n0 >= g.N) return;   // a wave whose whole tile is outside (no barrier in this kernel)
    MxRows<FW, TN> wr;
    MxRows<FA, TM> ar;
    wr.init(g.we, g.ws, n0, g.N, g.K, lane);
    ar.init(g.ae, g.as, m0, g.M, g.K, lane);

    f32x4_t acc[TN][TM];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) acc[tn][tm] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int64_t steps = g.K / 128;
    MxFrags<FW, TN> w0, w1;
    MxFrags<FA, TM> a0, a1;
    w0.load(wr, 0);
    a0.load(ar, 0);
    int64_t s = 0;
    for (; s + 2 <= steps; s += 2) {
        w1.load(wr, s + 1);
        a1.load(ar, s + 1);
        mx_mma<FW, FA>(acc, w0, a0);
        if (s + 2 < steps) {
            w0.load(wr, s + 2);
            a0.load(ar, s + 2);
        }
        mx_mma<FW, FA>(acc, w1, a1);
    }
    if (s < steps) {
        mx_mma<FW, FA>(acc, w0, a0);
    }
    const bool vec = (g.N & 3) == 0;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
            mx_store4(g.out, m0 + 16 * tm + (lane & 15), n0 + 16 * tn + 4 * (lane >> 4), g.M, g.N, acc[tn][tm], g.out_dtype, vec);
}

// TM instruction tiles of A (M <= 16 * TM); grid.x = ceil(N / 16)
template <int FW, int FA, int TM>
__global__ __launch_bounds__(64 * MXG_SKINNY_WAVES) void mx_gemm_skinny(MxGemmArgs g) {
    constexpr int WV = MXG_SKINNY_WAVES, U = 4;   // U K steps in flight per wave
    __shared__ float part[WV][TM][64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    MxRows<FW, 1> wr;
    MxRows<FA, TM> ar;
    wr.init(g.we, g.ws, n0, g.N, g.K, lane);
    ar.init(g.ae, g.as, 0, g.M, g.K, lane);

    f32x4_t acc[1][TM];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm) acc[0][tm] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int64_t steps = g.K / 128;
    for (int64_t s = wave; s < steps; s += WV * U) {
        MxFrags<FW, 1> w[U];
        MxFrags<FA, TM> a[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t su = s + u * WV;
            const int64_t sl = su < steps ? su : steps - 1;   // a step past the end re-loads the last one and is not used
            w[u].load(wr, sl);
            a[u].load(ar, sl);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (s + u * WV < steps) {   // wave-uniform
                mx_mma<FW, FA>(acc, w[u], a[u]);
            }
        }
    }
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[wave][tm][lane][i] = acc[0][tm][i];
    __syncthreads();
    // one result per thread, the 8 partial sums added in wave order
    for (int e = threadIdx.x; e < TM * 256; e += 64 * WV) {
        const int tm = e >> 8, l = (e >> 2) & 63, i = e & 3;
        float v = part[0][tm][l][i];
#pragma unroll
        for (int w = 1; w < WV; ++w) v += part[w][tm][l][i];
        const int64_t m = 16 * tm + (l & 15), n = n0 + 4 * (l >> 4) + i;
        if (m < g.M && n < g.N) mx_store1(g.out, m * g.N + n, v, g.out_dtype);
    }
}

// instruction format code of an FQ_MX_* export format
constexpr int mxg_code(int fmt) { return fmt == 0 ? 4 : fmt == 3 ? 0 : 1; }

template <int FW, int FA> static void launch_mx_gemm_pair(const MxGemmArgs& g, hipStream_t st) {
    if (g.M <= MXG_SKINNY_M) {
        const dim3 grid((unsigned)((g.N + 15) / 16));
        if (g.M <= 16) launch(mx_gemm_skinny<FW, FA, 1>, grid, dim3(64 * MXG_SKINNY_WAVES), st, g);
        else launch(mx_gemm_skinny<FW, FA, 2>, grid, dim3(64 * MXG_SKINNY_WAVES), st, g);
    } else {
        const dim3 grid((unsigned)((g.M + MXG_TILE - 1) / MXG_TILE), (unsigned)((g.N + MXG_TILE - 1) / MXG_TILE));
        launch(mx_gemm_tiled<FW, FA>, grid, dim3(256), st, g);
    }
}

template <int FW> static void launch_mx_gemm_w(const MxGemmArgs& g, hipStream_t st) {
    switch (mxg_code(g.a_fmt)) {
        case 4: launch_mx_gemm_pair<FW, 4>(g, st); break;
        case 0: launch_mx_gemm_pair<FW, 0>(g, st); break;
        default: launch_mx_gemm_pair<FW, 1>(g, st); break;
    }
}

// g validated by fq_mx_gemm: M, N > 0, K a positive multiple of 128, formats exportable, the grid within limits
int launch_mx_gemm(const MxGemmArgs& g, hipStream_t st) {
    begin_launches();
    switch (mxg_code(g.w_fmt)) {
        case 4: launch_mx_gemm_w<4>(g, st); break;
        case 0: launch_mx_gemm_w<0>(g, st); break;
        default: launch_mx_gemm_w<1>(g, st); break;
    }
    return launch_result();
}

}  // namespace fq
