// fq_loss_rows.h -- the row-softmax layer under the loss kernels: what fq_kd_loss.h (two logit tensors) and
// fq_ce_loss.h (one) share, and what a further loss over rows of logits would stand on.  A device part (constants, exponentials, the
// reference point, unpack / pack, the element path's group load, the reduction over a row's waves) and a host part (the entry points'
// common refusals, the launch shape, the access path).  Retuning a constant here retunes every loss.
//
// Launch shape (every row kernel of a loss): rows of LOSS_WIDE elements or more take a 256-thread workgroup each (TPR = 256) and loop
// over sweeps; shorter rows take one wave each, four to a workgroup (TPR = 64, no LDS, no barrier), as the row kernels' launch-shape
// table does.  VEC: 16-byte loads and stores, where the base pointers are 16-byte aligned and a row is whole vectors; else element
// accesses (any cols, any alignment: cols = 32001 is a real vocabulary), which feed the same arithmetic in groups of LOSS_EG strided
// elements.  Slots past the end of a row hold -inf: e^-inf = 0 adds nothing to a sum.
//
// Special values.  The reference point of a lane that has seen only -inf is 0 (loss_ref), so that -inf - max is never inf - inf; a
// row of only -inf ends in z = 0, and its loss is NaN as ATen's is.  v_max_f32 ignores a NaN operand, but e^(NaN - m) is NaN: the sum,
// hence the logsumexp, the row's loss and its gradient are NaN.  exp is v_exp_f32 on (x - m) * log2(e): the difference is taken first
// (exact or nearly so), so the argument's error is relative to the distance from the maximum, where the term's weight is small.
// Results below the fp32 normal range flush to zero.
#pragma once
#include "fq_launch.h"

namespace fq {

// ---- device part -----------------------------------------------------------------------------------------------------------------------
constexpr int LOSS_TPB = 256;          // threads per workgroup
constexpr int64_t LOSS_WIDE = 2048;    // cols from which a row takes the whole workgroup
constexpr int LOSS_EG = 4;             // elements per group of the element path
constexpr float LOSS_LOG2E = 1.44269504088896340736f;
#define LOSS_NEG_INF (-__builtin_inff())

struct OpAddF {   // a + b is commutative bit for bit, so the butterfly of wave_reduce gives every lane the same sum
    __device__ static __forceinline__ uint32_t f(uint32_t a, uint32_t b) { return as_u(as_f(a) + as_f(b)); }
};

__device__ __forceinline__ float loss_exp(float d) { return __builtin_amdgcn_exp2f(d * LOSS_LOG2E); }
// e^d for the gradient, where an element's relative error counts whatever its size: d * log2(e) as an unevaluated sum hi + lo (lo: the
// product's rounding error and the fp32 constant's own, both proportional to |d|, which loss_exp leaves in the result as a relative error
// of about |d| 2^-24), v_exp_f32 on hi, lo applied to first order.  d = -inf: hi = -inf, lo = NaN, and the result is the 0 of 2^hi.
constexpr float LOSS_LOG2E_LO = 1.92596299e-8f;     // log2(e) - (float)log2(e)
constexpr float LOSS_LN2 = 0.693147180559945309417f;
__device__ __forceinline__ float loss_exp_acc(float d) {
    const float hi = d * LOSS_LOG2E;
    const float lo = __builtin_fmaf(d, LOSS_LOG2E_LO, __builtin_fmaf(d, LOSS_LOG2E, -hi));
    const float e = __builtin_amdgcn_exp2f(hi);
    return e == 0.0f ? 0.0f : __builtin_fmaf(e, lo * LOSS_LN2, e);
}
__device__ __forceinline__ float loss_ref(float m) { return m == LOSS_NEG_INF ? 0.0f : m; }

// the row and the lane's place in it -> false: no such row (RPB > 1 only: a whole wave, and those rows meet no barrier)
template <int TPR> __device__ __forceinline__ bool loss_row_lane(int64_t rows, int64_t& row, int& lane) {
    lane = threadIdx.x & (TPR - 1);
    row = (int64_t)blockIdx.x * (LOSS_TPB / TPR) + threadIdx.x / TPR;
    return row < rows;
}

// a 16-byte vector as floats, and back (rounded once to the dtype)
template <int DT> __device__ __forceinline__ void loss_unpack(const uint4& v, float (&f)[16 / Ty<DT>::ESIZE]) {
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
template <int DT> __device__ __forceinline__ uint4 loss_pack(const float (&f)[16 / Ty<DT>::ESIZE]) {
    using T = Ty<DT>;
    uint32_t o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        float e[T::EPD];
#pragma unroll
        for (int k = 0; k < T::EPD; ++k) e[k] = f[d * T::EPD + k];
        o[d] = T::pack(e);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// the element path's group: columns c, c + TPR, ... of the row that starts at element `base` of p; a slot past the row is -inf, and its
// address the group's first (c < cols)
template <int DT, int TPR> __device__ __forceinline__ void loss_load_group(const void* p, int64_t base, int64_t c, int64_t cols, float (&f)[LOSS_EG]) {
#pragma unroll
    for (int i = 0; i < LOSS_EG; ++i) {
        const int64_t ci = c + i * TPR;
        const bool in = ci < cols;
        const float x = Ty<DT>::load1(p, base + (in ? ci : c));
        f[i] = in ? x : LOSS_NEG_INF;
    }
}

// K values reduced over the row's NW waves with one barrier; lds is [K][4], used by this call alone
template <class Op, int NW, int K> __device__ __forceinline__ void loss_reduce(uint32_t (&v)[K], uint32_t (*lds)[4]) {
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

// ---- host part -------------------------------------------------------------------------------------------------------------------------
constexpr int LOSS_CONTINUE = 1;

// what every loss entry point checks first, in the headers' order: LOSS_CONTINUE, or the refusal.  Every check comes before any HIP call.
inline int loss_head(int64_t rows, int64_t cols, int dtype) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the loss entry points");
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return fail(FQ_ERR_SHAPE, "empty shape rows=%lld cols=%lld: a loss has no empty launch", (long long)rows, (long long)cols);
    if (rows > INT64_MAX / 4 / cols) return fail(FQ_ERR_SHAPE, "rows * cols overflows");
    return LOSS_CONTINUE;
}

// rows of LOSS_WIDE elements or more: a workgroup each; shorter ones: a wave each, four to a workgroup
inline bool loss_wide(int64_t cols) { return cols >= LOSS_WIDE; }
inline int64_t loss_grid(int64_t rows, int64_t cols) { return loss_wide(cols) ? rows : (rows + 3) / 4; }
inline int loss_grid_check(int64_t rows, int64_t cols) {
    if (loss_grid(rows, cols) > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "%lld rows exceed one launch's grid", (long long)rows);
    return LOSS_CONTINUE;
}
// 16-byte accesses: every row of every tensor starts on a 16-byte boundary and is whole vectors
inline bool loss_vec(int64_t cols, int dtype, const void* p0, const void* p1 = nullptr, const void* p2 = nullptr) {
    return aligned16(p0) && aligned16(p1) && aligned16(p2) && cols * esize_of(dtype) % 16 == 0;
}
// the (wide, vec) ladder of a row kernel <DT, VEC, TPR>: f(VEC as 0 / 1, TPR), for launch_rows<TPR> (whose grid is loss_grid)
static_assert(LOSS_TPB == 256, "launch_rows<64 / 256> launches 256-thread workgroups");
template <class F> inline void by_loss_shape(int64_t cols, bool vec, F&& f) {
    if (loss_wide(cols)) {
        if (vec) f(Const<1>{}, Const<256>{});
        else f(Const<0>{}, Const<256>{});
    } else {
        if (vec) f(Const<1>{}, Const<64>{});
        else f(Const<0>{}, Const<64>{});
    }
}

}  // namespace fq
