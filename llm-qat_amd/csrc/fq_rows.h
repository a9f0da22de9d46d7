// fq_rows.h -- the row layer under the loss and norm kernels: what is true of any kernel that gives a row to one
// wave or to one workgroup and reads it in 16-byte vectors or by elements.  fq_loss_rows.h (the softmax part, under fq_kd_loss.h and
// fq_ce_loss.h) and fq_rms_norm.h stand on it, and a further loss or norm over rows would.  A device part (the sizes, the row / lane
// prologue, unpack / pack, the element path's group load, the reduction over a row's waves) and a host part (the entry points' common
// refusals, the launch shape, the access path).  Retuning a constant here retunes every loss and the norm.
//
// Launch shape (every row kernel above this layer): rows of ROW_WIDE elements or more take a 256-thread workgroup each (TPR = 256) and
// loop over sweeps; shorter rows take one wave each, four to a workgroup (TPR = 64, no LDS, no barrier), as the row kernels' launch-shape
// table does.  VEC: 16-byte loads and stores, where the base pointers are 16-byte aligned and a row is whole vectors; else element
// accesses (any cols, any alignment: cols = 32001 is a real vocabulary), which feed the same arithmetic in groups of strided elements.
// A slot past the end of a row holds the caller's fill value, the one that adds nothing to its sums.
#pragma once
#include "fq_launch.h"

namespace fq {

// ---- device part -----------------------------------------------------------------------------------------------------------------------
constexpr int ROW_TPB = 256;           // threads per workgroup
constexpr int64_t ROW_WIDE = 2048;     // cols from which a row takes the whole workgroup

struct OpAddF {   // a + b is commutative bit for bit, so the butterfly of wave_reduce gives every lane the same sum
    __device__ static __forceinline__ uint32_t f(uint32_t a, uint32_t b) { return as_u(as_f(a) + as_f(b)); }
};

// the row and the lane's place in it -> false: no such row (RPB > 1 only: a whole wave, and those rows meet no barrier)
// (not fq_kernels.h's row_and_lane: that one returns true for TPR = 256 without a test, and through it the 56 TPR = 256 kernels above
// this layer differ: they lose the exit they never take, and up to 18 VGPRs with it)
template <int TPR> __device__ __forceinline__ bool row_lane(int64_t rows, int64_t& row, int& lane) {
    lane = threadIdx.x & (TPR - 1);
    row = (int64_t)blockIdx.x * (ROW_TPB / TPR) + threadIdx.x / TPR;
    return row < rows;
}

// a 16-byte vector as floats, and back (rounded once to the dtype)
template <int DT> __device__ __forceinline__ void row_unpack(const uint4& v, float (&f)[16 / Ty<DT>::ESIZE]) {
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
template <int DT> __device__ __forceinline__ uint4 row_pack(const float (&f)[16 / Ty<DT>::ESIZE]) {
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

// the element path's group: columns c, c + TPR, ... of the row that starts at element `base` of p; a slot past the row is `fill`, and its
// address the group's first (c < cols)
template <int DT, int TPR, int N>
__device__ __forceinline__ void row_load_group(const void* p, int64_t base, int64_t c, int64_t cols, float fill, float (&f)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int64_t ci = c + i * TPR;
        const bool in = ci < cols;
        const float x = Ty<DT>::load1(p, base + (in ? ci : c));
        f[i] = in ? x : fill;
    }
}

// K values reduced over the row's NW waves with one barrier; lds is [K][4], used by this call alone
template <class Op, int NW, int K> __device__ __forceinline__ void row_reduce(uint32_t (&v)[K], uint32_t (*lds)[4]) {
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
constexpr int ROW_CONTINUE = 1;

// what every entry point above this layer checks first, in the headers' order: ROW_CONTINUE, or the refusal.  Every check comes before
// any HIP call.  noun: what the messages call the family ("loss", "norm"); dtypes: its one or two dtype codes; between: the family's own
// dtype refusals, which the headers place behind the common ones and before the shape's (-> ROW_CONTINUE, or the refusal).  noun NULL is a
// size query's question, "is this shape served": no dtypes, and the answer without a message
template <class Between = int (*)()>
inline int row_head(const char* noun, int64_t rows, int64_t cols, std::initializer_list<int> dtypes = {}, Between&& between = [] { return ROW_CONTINUE; }) {
    for (const int dt : dtypes) {
        if (dt < 0 || dt > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dt);
        if (dt == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the %s entry points", noun);
    }
    if (const int rc = between(); rc != ROW_CONTINUE) return rc;
    if (rows > 0 && cols > 0 && rows <= INT64_MAX / 4 / cols) return ROW_CONTINUE;
    if (!noun) return FQ_ERR_SHAPE;
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return fail(FQ_ERR_SHAPE, "empty shape rows=%lld cols=%lld: a %s has no empty launch", (long long)rows, (long long)cols, noun);
    return fail(FQ_ERR_SHAPE, "rows * cols overflows");
}

// rows of ROW_WIDE elements or more: a workgroup each; shorter ones: a wave each, four to a workgroup
inline bool row_wide(int64_t cols) { return cols >= ROW_WIDE; }
inline int64_t row_grid(int64_t rows, int64_t cols) { return row_wide(cols) ? rows : (rows + 3) / 4; }
inline int row_grid_check(int64_t rows, int64_t cols) {
    if (row_grid(rows, cols) > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "%lld rows exceed one launch's grid", (long long)rows);
    return ROW_CONTINUE;
}
// 16-byte accesses: every row of every tensor starts on a 16-byte boundary and is whole vectors
inline bool row_vec(int64_t cols, int dtype, const void* p0, const void* p1 = nullptr, const void* p2 = nullptr) {
    return aligned16(p0) && aligned16(p1) && aligned16(p2) && cols * esize_of(dtype) % 16 == 0;
}
// the (wide, vec) ladder of a row kernel <DT, VEC, TPR>: f(VEC as 0 / 1, TPR), for launch_rows<TPR> (whose grid is row_grid)
static_assert(ROW_TPB == 256, "launch_rows<64 / 256> launches 256-thread workgroups");
template <class F> inline void by_row_shape(int64_t cols, bool vec, F&& f) {
    if (row_wide(cols)) {
        if (vec) f(Const<1>{}, Const<256>{});
        else f(Const<0>{}, Const<256>{});
    } else {
        if (vec) f(Const<1>{}, Const<64>{});
        else f(Const<0>{}, Const<64>{});
    }
}

}  // namespace fq
