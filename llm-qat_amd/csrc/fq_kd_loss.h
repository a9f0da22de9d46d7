// fq_kd_loss.h -- the distillation loss kl_div(log_softmax(s), softmax(t), "batchmean") and its gradient: the
// kernels behind include/llmqat_fakequant_loss.h.  fp32 arithmetic whatever the logits' dtype; no fp32 [rows, cols] tensor ever exists.
//
//   kd_fwd_kernel   one pass over a row of s and t with an online softmax.  A lane's running state is
//                       ms, zs = max and sum e^(s - ms) of the student elements it has seen;  mt, zt the teacher's;
//                       a = sum e^(t - mt) (t - s)
//                   rebased (kd_rebase) once per 16-byte vector to the vector's maxima, not once per element.  At the end of the row
//                   the lanes rebase to the row's maxima (max-reduce), their zs, zt, a are summed (DPP butterfly, then across the
//                   waves through LDS in wave order: a fixed order, no atomics), and with ls = log zs, lt = log zt
//                       lse_s = ms + ls,  lse_t = mt + lt,  row_loss = (a / zt - lse_t) + lse_s
//                   which is sum p_t (t - s) - lse_t + lse_s term for term: each of the three is rounded at its own size, the sizes
//                   the error measure of tests/kd_loss_reference.py adds up (taking the differences against the maxima instead,
//                   (t - mt) - (s - ms), saves nothing where the two maxima differ: the first term then carries mt - ms).
//                   Student and teacher go through the same code, so kd(s, s) has a == 0 and lse_s == lse_t exactly: row_loss is 0.0.
//   kd_sum_kernel   one workgroup: the row losses summed in float64 in a fixed order, divided by the batch, rounded to fp32.
//   kd_bwd_kernel   one pass: grad = (g / batch) (e^(s - lse_s) - e^(t - lse_t)), rounded once to the dtype (kd_exp_acc: the product
//                   with log2(e) carried to twice the precision).
//
// Launch shape (both row kernels): rows of 2048 elements or more take a 256-thread workgroup each (TPR = 256) and loop over sweeps; shorter
// rows take one wave each, four to a workgroup (TPR = 64, no LDS, no barrier), as the row kernels' launch-shape table does.  VEC: 16-byte
// loads and stores, where the base pointers are 16-byte aligned and a row is whole vectors; else element accesses (any cols, any
// alignment: cols = 32001 is a real vocabulary), which feed the same arithmetic in groups of KD_EG strided elements.  Slots past the end
// of a row hold -inf in both tensors: e^-inf = 0 adds nothing to a sum, and a term whose e^(t - mt) is 0 is dropped (below).
//
// Special values.  A term is dropped where e^(t - mt) == 0 (kl_div's xlogy rule: p_t == 0 contributes 0; here also where s is -inf,
// the one deviation from ATen, which gives NaN for -inf in both).  s = -inf under e^(t - mt) > 0 gives a = +inf.  The reference point
// of a lane that has seen only -inf is 0 (kd_ref), so that -inf - max is never inf - inf; a row of only -inf ends in 0 / 0 = NaN as
// ATen's does.  v_max_f32 ignores a NaN operand, but e^(NaN - m) is NaN: zs or zt, hence lse, the row's loss and its gradient are NaN.
// exp is v_exp_f32 on (x - m) * log2(e): the difference is taken first (exact or nearly so), so the argument's error is relative to the
// distance from the maximum, where the term's weight is small.  Results below the fp32 normal range flush to zero.
#pragma once
#include "fq_launch.h"

#ifndef KD_NT_LOAD
#define KD_NT_LOAD 0     // the logits were written by the GEMM just before and are read again by the backward
#endif
#ifndef KD_NT_STORE
#define KD_NT_STORE 1
#endif

namespace fq {

constexpr int KD_TPB = 256;          // threads per workgroup
constexpr int64_t KD_WIDE = 2048;    // cols from which a row takes the whole workgroup
constexpr int KD_EG = 4;             // elements per group of the element path
constexpr float KD_LOG2E = 1.44269504088896340736f;
#define KD_NEG_INF (-__builtin_inff())

struct KdFwdArgs {
    const void* s;
    const void* t;
    float* stats;      // [rows, 2] or nullptr
    float* row_loss;   // [rows]
    int64_t rows, cols;
};
struct KdBwdArgs {
    const void* s;
    const void* t;
    const float* stats;
    const float* g;    // the upstream gradient: one float on the device
    void* gs;
    int64_t rows, cols;
    float batch;
};

struct OpAddF {   // a + b is commutative bit for bit, so the butterfly of wave_reduce gives every lane the same sum
    __device__ static __forceinline__ uint32_t f(uint32_t a, uint32_t b) { return as_u(as_f(a) + as_f(b)); }
};

__device__ __forceinline__ float kd_exp(float d) { return __builtin_amdgcn_exp2f(d * KD_LOG2E); }
// e^d for the gradient, where an element's relative error counts whatever its size: d * log2(e) as an unevaluated sum hi + lo (lo: the
// product's rounding error and the fp32 constant's own, both proportional to |d|, which kd_exp leaves in the result as a relative error of
// about |d| 2^-24), v_exp_f32 on hi, lo applied to first order.  d = -inf: hi = -inf, lo = NaN, and the result is the 0 of 2^hi.
constexpr float KD_LOG2E_LO = 1.92596299e-8f;     // log2(e) - (float)log2(e)
constexpr float KD_LN2 = 0.693147180559945309417f;
__device__ __forceinline__ float kd_exp_acc(float d) {
    const float hi = d * KD_LOG2E;
    const float lo = __builtin_fmaf(d, KD_LOG2E_LO, __builtin_fmaf(d, KD_LOG2E, -hi));
    const float e = __builtin_amdgcn_exp2f(hi);
    return e == 0.0f ? 0.0f : __builtin_fmaf(e, lo * KD_LN2, e);
}
__device__ __forceinline__ float kd_ref(float m) { return m == KD_NEG_INF ? 0.0f : m; }

struct KdState {
    float ms = KD_NEG_INF, zs = 0.0f, mt = KD_NEG_INF, zt = 0.0f, a = 0.0f;
};
// the state re-expressed against the maxima ms >= st.ms, mt >= st.mt.  A side that has seen nothing finite holds z == 0 (and a == 0 on
// the teacher's): its factor is 0, not e^(0 - new reference), which may be inf.  A teacher factor that underflows takes a's terms with it,
// an infinite one (s = -inf) included: their p_t is 0.
__device__ __forceinline__ void kd_rebase(KdState& st, float ms, float mt) {
    const float ds = kd_ref(st.ms) - kd_ref(ms), dt = kd_ref(st.mt) - kd_ref(mt);
    const float fs = st.ms == KD_NEG_INF ? 0.0f : kd_exp(ds), ft = st.mt == KD_NEG_INF ? 0.0f : kd_exp(dt);
    st.a = ft == 0.0f ? 0.0f : ft * st.a;
    st.zs *= fs;
    st.zt *= ft;
    st.ms = ms;
    st.mt = mt;
}
template <int N> __device__ __forceinline__ void kd_accumulate(KdState& st, const float (&s)[N], const float (&t)[N]) {
    float vs = s[0], vt = t[0];
#pragma unroll
    for (int i = 1; i < N; ++i) vs = __builtin_fmaxf(vs, s[i]), vt = __builtin_fmaxf(vt, t[i]);
    kd_rebase(st, __builtin_fmaxf(st.ms, vs), __builtin_fmaxf(st.mt, vt));
    const float rs = kd_ref(st.ms), rt = kd_ref(st.mt);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float ds = s[i] - rs, dt = t[i] - rt;
        const float es = kd_exp(ds), et = kd_exp(dt);
        st.zs += es;
        st.zt += et;
        const float term = et * (t[i] - s[i]);
        st.a += et == 0.0f ? 0.0f : term;
    }
}
template <int DT> __device__ __forceinline__ void kd_unpack(const uint4& v, float (&f)[16 / Ty<DT>::ESIZE]) {
    using T = Ty<DT>;
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        float e[T::EPD];
        T::unpack(w[d], e);
#pragma unroll
        for (int k = 0; k < T::EPD; ++k) f[d * T::EPD + k] = e[k];
    }
}

// K values reduced over the row's NW waves with one barrier; lds is [K][4], used by this call alone
template <class Op, int NW, int K> __device__ __forceinline__ void kd_reduce(uint32_t (&v)[K], uint32_t (*lds)[4]) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_reduce<Op>(v[k]);
    if constexpr (NW > 1) {
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) lds[k][wave] = v[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t r = lds[k][0];
#pragma unroll
            for (int i = 1; i < NW; ++i) r = Op::f(r, lds[k][i]);
            v[k] = r;
        }
    }
}

template <int DT, bool VEC, int TPR>
__global__ __launch_bounds__(KD_TPB) void kd_fwd_kernel(KdFwdArgs a) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE, RPB = KD_TPB / TPR, NW = TPR / 64;
    __shared__ uint32_t lds_max[2][4], lds_sum[3][4];
    const int lane = threadIdx.x & (TPR - 1);
    const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
    if (row >= a.rows) return;      // RPB > 1 only: a whole wave, and those rows meet no barrier
    const int64_t base = row * a.cols;
    KdState st;
    if constexpr (VEC) {
        const uint4* ps = (const uint4*)((const char*)a.s + base * T::ESIZE);
        const uint4* pt = (const uint4*)((const char*)a.t + base * T::ESIZE);
        const int64_t nvec = a.cols / EPV;
        for (int64_t v = lane; v < nvec; v += 2 * TPR) {     // two vectors of each tensor in flight
            const int64_t v1 = v + TPR;
            const bool more = v1 < nvec;
            const uint4 s0 = ld16<KD_NT_LOAD != 0>(ps + v), t0 = ld16<KD_NT_LOAD != 0>(pt + v);
            const uint4 s1 = ld16<KD_NT_LOAD != 0>(ps + (more ? v1 : v)), t1 = ld16<KD_NT_LOAD != 0>(pt + (more ? v1 : v));
            float fs[EPV], ft[EPV];
            kd_unpack<DT>(s0, fs);
            kd_unpack<DT>(t0, ft);
            kd_accumulate(st, fs, ft);
            if (more) {
                kd_unpack<DT>(s1, fs);
                kd_unpack<DT>(t1, ft);
                kd_accumulate(st, fs, ft);
            }
        }
    } else {
        for (int64_t c = lane; c < a.cols; c += KD_EG * TPR) {
            float fs[KD_EG], ft[KD_EG];
#pragma unroll
            for (int i = 0; i < KD_EG; ++i) {
                const int64_t ci = c + i * TPR;
                const bool in = ci < a.cols;
                const float xs = T::load1(a.s, base + (in ? ci : c)), xt = T::load1(a.t, base + (in ? ci : c));
                fs[i] = in ? xs : KD_NEG_INF;
                ft[i] = in ? xt : KD_NEG_INF;
            }
            kd_accumulate(st, fs, ft);
        }
    }
    uint32_t m[2] = {as_u(st.ms), as_u(st.mt)};
    kd_reduce<OpMaxF, NW>(m, lds_max);
    kd_rebase(st, as_f(m[0]), as_f(m[1]));
    uint32_t z[3] = {as_u(st.zs), as_u(st.zt), as_u(st.a)};
    kd_reduce<OpAddF, NW>(z, lds_sum);
    if (lane == 0) {
        const float zs = as_f(z[0]), zt = as_f(z[1]);
        const float lse_s = kd_ref(st.ms) + __builtin_logf(zs), lse_t = kd_ref(st.mt) + __builtin_logf(zt);
        if (a.stats) {
            a.stats[2 * row] = lse_s;
            a.stats[2 * row + 1] = lse_t;
        }
        a.row_loss[row] = (as_f(z[2]) / zt - lse_t) + lse_s;
    }
}

__global__ __launch_bounds__(KD_TPB) void kd_sum_kernel(const float* row_loss, float* loss, int64_t rows, double batch) {
    __shared__ double sh[KD_TPB];
    double acc = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += KD_TPB) acc += (double)row_loss[r];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = KD_TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(sh[0] / batch);
}

template <int N> __device__ __forceinline__ void kd_grad(float (&s)[N], const float (&t)[N], float lse_s, float lse_t, float gb) {
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = gb * (kd_exp_acc(s[i] - lse_s) - kd_exp_acc(t[i] - lse_t));
}
template <int DT> __device__ __forceinline__ uint4 kd_grad_vec(const uint4& s, const uint4& t, float lse_s, float lse_t, float gb) {
    using T = Ty<DT>;
    float fs[16 / T::ESIZE], ft[16 / T::ESIZE];
    kd_unpack<DT>(s, fs);
    kd_unpack<DT>(t, ft);
    kd_grad(fs, ft, lse_s, lse_t, gb);
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        float e[T::EPD];
#pragma unroll
        for (int k = 0; k < T::EPD; ++k) e[k] = fs[d * T::EPD + k];
        o[d] = T::pack(e);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

template <int DT, bool VEC, int TPR>
__global__ __launch_bounds__(KD_TPB) void kd_bwd_kernel(KdBwdArgs a) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE, RPB = KD_TPB / TPR;
    const int lane = threadIdx.x & (TPR - 1);
    const int64_t row = (int64_t)blockIdx.x * RPB + threadIdx.x / TPR;
    if (row >= a.rows) return;
    const int64_t base = row * a.cols;
    const float lse_s = a.stats[2 * row], lse_t = a.stats[2 * row + 1], gb = a.g[0] / a.batch;
    if constexpr (VEC) {
        const uint4* ps = (const uint4*)((const char*)a.s + base * T::ESIZE);
        const uint4* pt = (const uint4*)((const char*)a.t + base * T::ESIZE);
        uint4* pg = (uint4*)((char*)a.gs + base * T::ESIZE);
        const int64_t nvec = a.cols / EPV;
        for (int64_t v = lane; v < nvec; v += 2 * TPR) {
            const int64_t v1 = v + TPR;
            const bool more = v1 < nvec;
            const uint4 s0 = ld16<KD_NT_LOAD != 0>(ps + v), t0 = ld16<KD_NT_LOAD != 0>(pt + v);
            const uint4 s1 = ld16<KD_NT_LOAD != 0>(ps + (more ? v1 : v)), t1 = ld16<KD_NT_LOAD != 0>(pt + (more ? v1 : v));
            st16<KD_NT_STORE != 0>(pg + v, kd_grad_vec<DT>(s0, t0, lse_s, lse_t, gb));
            if (more) st16<KD_NT_STORE != 0>(pg + v1, kd_grad_vec<DT>(s1, t1, lse_s, lse_t, gb));
        }
    } else {
        for (int64_t c = lane; c < a.cols; c += TPR) {
            float fs[1] = {T::load1(a.s, base + c)}, ft[1] = {T::load1(a.t, base + c)};
            kd_grad(fs, ft, lse_s, lse_t, gb);
            T::store1(a.gs, base + c, fs[0]);
        }
    }
}

}  // namespace fq
