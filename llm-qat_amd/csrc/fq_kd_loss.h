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
//   kd_bwd_kernel   one pass: grad = (g / batch) (e^(s - lse_s) - e^(t - lse_t)), rounded once to the dtype (loss_exp_acc: the product
//                   with log2(e) carried to twice the precision).
//
// Launch shape and access paths are the row layer's (fq_rows.h), the exponentials and the reference point the softmax layer's
// (fq_loss_rows.h).  Slots past the end of a row hold -inf in both tensors: e^-inf = 0 adds nothing to a sum, and a term whose
// e^(t - mt) is 0 is dropped:
//
// Special values of this loss.  A term is dropped where e^(t - mt) == 0 (kl_div's xlogy rule: p_t == 0 contributes 0; here also where s is
// -inf, the one deviation from ATen, which gives NaN for -inf in both).  s = -inf under e^(t - mt) > 0 gives a = +inf.  A row of only
// -inf ends in 0 / 0 = NaN as ATen's does.  A NaN element makes zs or zt, hence lse, the row's loss and its gradient NaN.
#pragma once
#include "fq_loss_rows.h"

#ifndef KD_NT_LOAD
#define KD_NT_LOAD 0     // the logits were written by the GEMM just before and are read again by the backward
#endif
#ifndef KD_NT_STORE
#define KD_NT_STORE 1
#endif

namespace fq {

constexpr int KD_SUM_TPB = 256;        // threads of the one workgroup that sums the rows: it fixes the order of the sum

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

struct KdState {
    float ms = LOSS_NEG_INF, zs = 0.0f, mt = LOSS_NEG_INF, zt = 0.0f, a = 0.0f;
};
// the state re-expressed against the maxima ms >= st.ms, mt >= st.mt.  A side that has seen nothing finite holds z == 0 (and a == 0 on
// the teacher's): its factor is 0, not e^(0 - new reference), which may be inf.  A teacher factor that underflows takes a's terms with it,
// an infinite one (s = -inf) included: their p_t is 0.
__device__ __forceinline__ void kd_rebase(KdState& st, float ms, float mt) {
    const float ds = loss_ref(st.ms) - loss_ref(ms), dt = loss_ref(st.mt) - loss_ref(mt);
    const float fs = st.ms == LOSS_NEG_INF ? 0.0f : loss_exp(ds), ft = st.mt == LOSS_NEG_INF ? 0.0f : loss_exp(dt);
    st.a = ft == 0.0f ? 0.0f : ft * st.a;
    st.zs *= fs;
    st.zt *= ft;
    st.ms = ms;
    st.mt = mt;
}
// (not one form with ce_accumulate: each exponential is added into the running sum here, the vector's are summed first there, and either
// order in the other's place changes its bits)
template <int N> __device__ __forceinline__ void kd_accumulate(KdState& st, const float (&s)[N], const float (&t)[N]) {
    float vs = s[0], vt = t[0];
#pragma unroll
    for (int i = 1; i < N; ++i) vs = __builtin_fmaxf(vs, s[i]), vt = __builtin_fmaxf(vt, t[i]);
    kd_rebase(st, __builtin_fmaxf(st.ms, vs), __builtin_fmaxf(st.mt, vt));
    const float rs = loss_ref(st.ms), rt = loss_ref(st.mt);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const float ds = s[i] - rs, dt = t[i] - rt;
        const float es = loss_exp(ds), et = loss_exp(dt);
        st.zs += es;
        st.zt += et;
        const float term = et * (t[i] - s[i]);
        st.a += et == 0.0f ? 0.0f : term;
    }
}

template <int DT, bool VEC, int TPR>
__global__ __launch_bounds__(ROW_TPB) void kd_fwd_kernel(KdFwdArgs a) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE, NW = TPR / 64;
    __shared__ uint32_t lds_max[2][4], lds_sum[3][4];
    int64_t row;
    int lane;
    if (!row_lane<TPR>(a.rows, row, lane)) return;
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
            row_unpack<DT>(s0, fs);
            row_unpack<DT>(t0, ft);
            kd_accumulate(st, fs, ft);
            if (more) {
                row_unpack<DT>(s1, fs);
                row_unpack<DT>(t1, ft);
                kd_accumulate(st, fs, ft);
            }
        }
    } else {
        for (int64_t c = lane; c < a.cols; c += LOSS_EG * TPR) {
            float fs[LOSS_EG], ft[LOSS_EG];
            // (row_load_group written out for two tensors: through the helper, per tensor or per slot, the s and t loads of a slot are
            // no longer issued together and the six VEC = false instantiations take 39 VGPRs for 37)
#pragma unroll
            for (int i = 0; i < LOSS_EG; ++i) {
                const int64_t ci = c + i * TPR;
                const bool in = ci < a.cols;
                const float xs = T::load1(a.s, base + (in ? ci : c)), xt = T::load1(a.t, base + (in ? ci : c));
                fs[i] = in ? xs : LOSS_NEG_INF;
                ft[i] = in ? xt : LOSS_NEG_INF;
            }
            kd_accumulate(st, fs, ft);
        }
    }
    uint32_t m[2] = {as_u(st.ms), as_u(st.mt)};
    row_reduce<OpMaxF, NW>(m, lds_max);
    kd_rebase(st, as_f(m[0]), as_f(m[1]));
    uint32_t z[3] = {as_u(st.zs), as_u(st.zt), as_u(st.a)};
    row_reduce<OpAddF, NW>(z, lds_sum);
    if (lane == 0) {
        const float zs = as_f(z[0]), zt = as_f(z[1]);
        const float lse_s = loss_ref(st.ms) + __builtin_logf(zs), lse_t = loss_ref(st.mt) + __builtin_logf(zt);
        if (a.stats) {
            a.stats[2 * row] = lse_s;
            a.stats[2 * row + 1] = lse_t;
        }
        a.row_loss[row] = (as_f(z[2]) / zt - lse_t) + lse_s;
    }
}

__global__ __launch_bounds__(KD_SUM_TPB) void kd_sum_kernel(const float* row_loss, float* loss, int64_t rows, double batch) {
    __shared__ double sh[KD_SUM_TPB];
    double acc = 0.0;
    for (int64_t r = threadIdx.x; r < rows; r += KD_SUM_TPB) acc += (double)row_loss[r];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = KD_SUM_TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(sh[0] / batch);
}

template <int N> __device__ __forceinline__ void kd_grad(float (&s)[N], const float (&t)[N], float lse_s, float lse_t, float gb) {
#pragma unroll
    for (int i = 0; i < N; ++i) s[i] = gb * (loss_exp_acc(s[i] - lse_s) - loss_exp_acc(t[i] - lse_t));
}
template <int DT> __device__ __forceinline__ uint4 kd_grad_vec(const uint4& s, const uint4& t, float lse_s, float lse_t, float gb) {
    using T = Ty<DT>;
    float fs[16 / T::ESIZE], ft[16 / T::ESIZE];
    row_unpack<DT>(s, fs);
    row_unpack<DT>(t, ft);
    kd_grad(fs, ft, lse_s, lse_t, gb);
    return row_pack<DT>(fs);
}

template <int DT, bool VEC, int TPR>
__global__ __launch_bounds__(ROW_TPB) void kd_bwd_kernel(KdBwdArgs a) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE;
    int64_t row;
    int lane;
    if (!row_lane<TPR>(a.rows, row, lane)) return;
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
