// fq_ce_loss.h -- the language-model loss cross_entropy(logits, labels, ignore_index) with the causal one-position shift done in the
// kernel, and its gradient: the kernels behind include/llmqat_fakequant_ce.h.  fp32 arithmetic whatever the
// logits' dtype; neither a shifted [B, T-1, V] copy nor an fp32 [rows, cols] tensor ever exists.  The simpler sibling of fq_kd_loss.h (one
// logit tensor instead of two); both stand on the row-softmax layer of fq_loss_rows.h, and that on the row layer of fq_rows.h.
//
//   ce_fwd_kernel   one pass over a row with an online logsumexp.  A lane's running state is m, z = max and sum e^(x - m) of the elements
//                   it has seen, rebased once per 16-byte vector to the vector's maximum (as kd_accumulate), not once per element.  At
//                   the end of the row the lanes rebase to the row's maximum (max-reduce), their z are summed (DPP butterfly, then across
//                   the waves through LDS in wave order: a fixed order, no atomics), and
//                       lse = m + log z,   row_loss = lse - x[y]
//                   The label's logit x[y] is fetched by lane 0 with one element load behind a range test of y: it is not looked for in
//                   the stream, and a label outside [0, cols) is never an address (the row's loss is NaN).
//   ce_sum_kernel   one workgroup: the row losses summed in float64 in a fixed order and the valid rows counted (int64), loss = sum / n
//                   ("mean": 0 / 0 = NaN when every row is ignored) or sum, rounded once to fp32; n is left on the device for the backward.
//   ce_bwd_kernel   one pass: grad = (g / n) (e^(x - lse) - [c == y]), rounded once to the dtype (loss_exp_acc).  The one-hot is applied
//                   per vector: one range test of the label's column against the vector's, taken by one lane of the row once.
//
// The effective label of row r (ce_label): labels[r], or with shift, labels[r + 1] for every row but the last of each sequence of
// seq_len rows, which is ignored: logits[..., :-1, :] against labels[..., 1:] on the unshifted pair.  rows % seq_len == 0 (the host
// checks), so r + 1 < rows wherever it is read.  An IGNORED ROW IS NEVER READ: the forward writes row_loss = 0 (and lse = 0) and returns,
// the backward stores zeros with the width it stores gradients with, so a NaN or inf there reaches nothing.
//
// Launch shape and access paths are the row layer's (fq_rows.h), the exponentials and the reference point the softmax layer's
// (fq_loss_rows.h).  A row is valid or ignored as a whole, and a row belongs to one wave (TPR = 64) or one workgroup (TPR = 256): the early
// return is uniform over whatever meets a barrier.
// CE_FWD_VIF / CE_BWD_VIF: 16-byte vectors a lane keeps in flight (A/B macros, as the two cache policies; DESIGN.md section 23 has the
// measurement).
//
// Special values of this loss.  A NaN element makes z, hence lse, the row's loss and its gradient NaN.  A row of only -inf has
// reference point 0 and z = 0: lse = -inf, row_loss = -inf - -inf = NaN, as ATen's.  x[y] = -inf under a
// finite lse gives +inf.  A row that is -inf but for a 0 at the label: m = 0, z = 1, lse = 0 + log 1 = 0, row_loss = 0 - 0 = 0.0 and
// the gradient e^0 - 1 = 0, e^-inf = 0 elsewhere.
#pragma once
#include "fq_loss_rows.h"

#ifndef CE_NT_LOAD
#define CE_NT_LOAD 0     // the logits were written by the GEMM just before and are read again by the backward
#endif
#ifndef CE_NT_STORE
#define CE_NT_STORE 1    // a plain store leaves the gradient dirty in the caches and slowed the kernel that ran next
#endif
#ifndef CE_FWD_VIF
#define CE_FWD_VIF 4
#endif
#ifndef CE_BWD_VIF
#define CE_BWD_VIF 4     // not 1: in that loop form the compiler drops the store's nt bit
#endif

namespace fq {

constexpr int CE_SUM_TPB = 1024;       // threads of the one workgroup that sums the rows
constexpr int CE_MEAN = 0, CE_SUM = 1; // FQC_REDUCTION_*
#define CE_NAN (__builtin_nanf(""))

struct CeLabels {
    const int64_t* labels;   // [rows]
    int64_t rows, seq_len, ignore_index;
    int shift;
};
struct CeFwdArgs {
    const void* x;
    CeLabels lab;
    float* row_lse;    // [rows] or nullptr
    float* row_loss;   // [rows]
    int64_t cols;
};
struct CeBwdArgs {
    const void* x;
    CeLabels lab;
    const float* row_lse;
    const int64_t* n_valid;
    const float* g;    // the upstream gradient: one float on the device
    void* gx;
    int64_t cols;
    int reduction;
};

// the effective label of `row` -> true: valid, y set (whatever its value: the callers range-test it); false: ignored
__device__ __forceinline__ bool ce_label(const CeLabels& l, int64_t row, int64_t& y) {
    if (l.shift) {
        // seq_len <= rows (it divides them): where the rows fit 32 bits, so does the remainder's arithmetic, at a fraction of the cost
        const bool last = (l.rows >> 32) == 0 ? (uint32_t)row % (uint32_t)l.seq_len == (uint32_t)l.seq_len - 1u
                                              : row % l.seq_len == l.seq_len - 1;
        if (last) return false;
        ++row;
    }
    y = l.labels[row];
    return y != l.ignore_index;
}

struct CeState {
    float m = LOSS_NEG_INF, z = 0.0f;
};
// the state re-expressed against the maximum m >= st.m; a lane that has seen nothing finite holds z == 0 and takes the factor 0, not
// e^(0 - m), which may be inf
__device__ __forceinline__ void ce_rebase(CeState& st, float m) {
    const float f = st.m == LOSS_NEG_INF ? 0.0f : loss_exp(loss_ref(st.m) - loss_ref(m));
    st.z *= f;
    st.m = m;
}
// (not one form with kd_accumulate: this one sums the vector's exponentials first and adds once, that one adds each into the running sum,
// and either order in the other's place changes its bits)
template <int N> __device__ __forceinline__ void ce_accumulate(CeState& st, const float (&x)[N]) {
    float vm = x[0];
#pragma unroll
    for (int i = 1; i < N; ++i) vm = __builtin_fmaxf(vm, x[i]);
    ce_rebase(st, __builtin_fmaxf(st.m, vm));
    const float r = loss_ref(st.m);
    float z = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) z += loss_exp(x[i] - r);
    st.z += z;
}

template <int DT, bool VEC, int TPR>
__global__ __launch_bounds__(ROW_TPB) void ce_fwd_kernel(CeFwdArgs a) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE, NW = TPR / 64, VIF = CE_FWD_VIF;
    constexpr uint32_t NEG_INF_WORD = DT == F32 ? 0xFF800000u : DT == BF16 ? 0xFF80FF80u : 0xFC00FC00u;   // -inf in every element of a dword
    __shared__ uint32_t lds_max[1][4], lds_sum[1][4];
    int64_t row;
    int lane;
    if (!row_lane<TPR>(a.lab.rows, row, lane)) return;
    int64_t y;
    if (!ce_label(a.lab, row, y)) {     // uniform over the row's lanes: nothing of the row is read
        if (lane == 0) {
            if (a.row_lse) a.row_lse[row] = 0.0f;
            a.row_loss[row] = 0.0f;
        }
        return;
    }
    const int64_t base = row * a.cols;
    float xy = CE_NAN;                  // a label outside [0, cols) is compared, never an address
    if (lane == 0 && y >= 0 && y < a.cols) xy = T::load1(a.x, base + y);
    CeState st;
    if constexpr (VEC) {
        const uint4* px = (const uint4*)((const char*)a.x + base * T::ESIZE);
        const int64_t nvec = a.cols / EPV;
        for (int64_t v = lane; v < nvec; v += VIF * TPR) {
            // every load is issued before the first use, and every use is unconditional (a use under a branch lets the compiler sink
            // its load into the branch, behind a wait of its own): a vector past the end of the row is replaced by -inf elements
            uint4 r[VIF];
#pragma unroll
            for (int i = 0; i < VIF; ++i) {
                const int64_t vi = v + i * TPR;
                r[i] = ld16<CE_NT_LOAD != 0>(px + (vi < nvec ? vi : v));
            }
#pragma unroll
            for (int i = 0; i < VIF; ++i) {
                if (i > 0 && v + i * TPR >= nvec) r[i] = make_uint4(NEG_INF_WORD, NEG_INF_WORD, NEG_INF_WORD, NEG_INF_WORD);
                float f[EPV];
                row_unpack<DT>(r[i], f);
                ce_accumulate(st, f);
            }
        }
    } else {
        for (int64_t c = lane; c < a.cols; c += LOSS_EG * TPR) {
            float f[LOSS_EG];
            row_load_group<DT, TPR>(a.x, base, c, a.cols, LOSS_NEG_INF, f);
            ce_accumulate(st, f);
        }
    }
    uint32_t m[1] = {as_u(st.m)};
    row_reduce<OpMaxF, NW>(m, lds_max);
    ce_rebase(st, as_f(m[0]));
    uint32_t z[1] = {as_u(st.z)};
    row_reduce<OpAddF, NW>(z, lds_sum);
    if (lane == 0) {
        const float lse = loss_ref(st.m) + __builtin_logf(as_f(z[0]));
        if (a.row_lse) a.row_lse[row] = lse;
        a.row_loss[row] = lse - xy;
    }
}

__global__ __launch_bounds__(CE_SUM_TPB) void ce_sum_kernel(const float* row_loss, CeLabels lab, float* loss, int64_t* n_valid, int reduction) {
    __shared__ double sh[CE_SUM_TPB];
    __shared__ int64_t cnt[CE_SUM_TPB];
    double acc = 0.0;
    int64_t n = 0;
    for (int64_t r = threadIdx.x; r < lab.rows; r += CE_SUM_TPB) {
        const float rl = row_loss[r];   // written for every row, 0.0 for an ignored one: loaded beside the label, not behind it
        int64_t y;
        const bool valid = ce_label(lab, r, y);
        acc += valid ? (double)rl : 0.0;
        n += valid ? 1 : 0;
    }
    sh[threadIdx.x] = acc;
    cnt[threadIdx.x] = n;
    __syncthreads();
    for (int s = CE_SUM_TPB / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh[threadIdx.x] += sh[threadIdx.x + s];
            cnt[threadIdx.x] += cnt[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *n_valid = cnt[0];
        *loss = (float)(reduction == CE_MEAN ? sh[0] / (double)cnt[0] : sh[0]);
    }
}

// e^(x - lse) in place, the 1 of the one-hot taken from slot `hot` (a slot of this vector, or anything else: no slot), times gn
template <int N> __device__ __forceinline__ void ce_grad(float (&x)[N], float lse, float gn, uint64_t hot) {
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = loss_exp_acc(x[i] - lse);
    if (hot < (uint64_t)N) {            // one test per vector; true for one lane of the row, once
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] -= (uint64_t)i == hot ? 1.0f : 0.0f;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] *= gn;
}
template <int DT> __device__ __forceinline__ uint4 ce_grad_vec(const uint4& x, float lse, float gn, uint64_t hot) {
    using T = Ty<DT>;
    float f[16 / T::ESIZE];
    row_unpack<DT>(x, f);
    ce_grad(f, lse, gn, hot);
    return row_pack<DT>(f);
}

template <int DT, bool VEC, int TPR>
__global__ __launch_bounds__(ROW_TPB) void ce_bwd_kernel(CeBwdArgs a) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE, VIF = CE_BWD_VIF;
    int64_t row;
    int lane;
    if (!row_lane<TPR>(a.lab.rows, row, lane)) return;
    const int64_t base = row * a.cols;
    int64_t y;
    if (!ce_label(a.lab, row, y)) {     // zeros, with the width the gradient is stored with; the row's logits are not read
        if constexpr (VEC) {
            uint4* pg = (uint4*)((char*)a.gx + base * T::ESIZE);
            const int64_t nvec = a.cols / EPV;
            for (int64_t v = lane; v < nvec; v += TPR) st16<CE_NT_STORE != 0>(pg + v, make_uint4(0u, 0u, 0u, 0u));
        } else {
            for (int64_t c = lane; c < a.cols; c += TPR) T::store1(a.gx, base + c, 0.0f);
        }
        return;
    }
    // a label outside [0, cols) matches no column; its row's gradient is NaN, as its loss
    const float lse = y >= 0 && y < a.cols ? a.row_lse[row] : CE_NAN;
    const float gn = a.reduction == CE_MEAN ? a.g[0] / (float)a.n_valid[0] : a.g[0];
    if constexpr (VEC) {
        const uint4* px = (const uint4*)((const char*)a.x + base * T::ESIZE);
        uint4* pg = (uint4*)((char*)a.gx + base * T::ESIZE);
        const int64_t nvec = a.cols / EPV;
        for (int64_t v = lane; v < nvec; v += VIF * TPR) {
            uint4 r[VIF];
#pragma unroll
            for (int i = 0; i < VIF; ++i) {
                const int64_t vi = v + i * TPR;
                r[i] = ld16<CE_NT_LOAD != 0>(px + (vi < nvec ? vi : v));
            }
#pragma unroll
            for (int i = 0; i < VIF; ++i) {
                const int64_t vi = v + i * TPR;
                if (i == 0 || vi < nvec) st16<CE_NT_STORE != 0>(pg + vi, ce_grad_vec<DT>(r[i], lse, gn, (uint64_t)(y - vi * EPV)));
            }
        }
    } else {
        for (int64_t c = lane; c < a.cols; c += LOSS_EG * TPR) {
            float f[LOSS_EG];
            // (not row_load_group: a slot past the row is never stored and holds the repeated element; the fill's select makes the six
            // VEC = false backwards differ, 32 -> 38 VGPRs)
#pragma unroll
            for (int i = 0; i < LOSS_EG; ++i) {
                const int64_t ci = c + i * TPR;
                f[i] = T::load1(a.x, base + (ci < a.cols ? ci : c));
            }
            // slot i of the group holds column c + i * TPR: the label's slot, if it is one of them
            const int64_t d = y - c;
            ce_grad(f, lse, gn, d >= 0 && d % TPR == 0 ? (uint64_t)(d / TPR) : ~(uint64_t)0);
#pragma unroll
            for (int i = 0; i < LOSS_EG; ++i) {
                const int64_t ci = c + i * TPR;
                if (ci < a.cols) T::store1(a.gx, base + ci, f[i]);
            }
        }
    }
}

}  // namespace fq
