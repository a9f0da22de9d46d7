// fq_swiglu.hip -- the SwiGLU kernels (fq_swiglu.h) and their entry points (include/llmqat_fakequant_act.h): a translation unit of its
// own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_act.h"

#include "fq_swiglu.h"

using namespace fq;

namespace {

// what both entry points check first, in the header's order: ROW_CONTINUE, or the refusal.  Every check comes before any HIP call.
int swi_head(int64_t rows, int64_t cols, std::initializer_list<int64_t> strides, int dtype) {
    if (const int rc = row_head("gated activation", rows, cols, {dtype}); rc != ROW_CONTINUE) return rc;
    for (const int64_t s : strides) {
        if (s < cols) return fail(FQ_ERR_SHAPE, "a row stride of %lld elements is below cols=%lld", (long long)s, (long long)cols);
        if (rows > 1 && s > (INT64_MAX / 4 - cols) / (rows - 1))
            return fail(FQ_ERR_SHAPE, "(rows - 1) * stride + cols overflows: rows=%lld stride=%lld", (long long)rows, (long long)s);
    }
    return ROW_CONTINUE;
}

// the walk and the access path of a launch, from the shape, the strides and the pointers: fills a's cols / strides / tpr -> the rows of
// the walk, vec: the 16-byte path
struct SwiWalk {
    int64_t rows;
    bool vec;
};
SwiWalk swi_walk(SwiGluArgs& a, int64_t rows, int64_t cols, int dtype, std::initializer_list<const void*> ptrs) {
    const bool flat = rows == 1 || (a.sg == cols && a.su == cols && (!a.dy || a.sdy == cols));
    const int64_t es = esize_of(dtype);
    bool vec = cols * es % 16 == 0;
    for (const void* p : ptrs) vec = vec && aligned16(p);
    if (!flat) vec = vec && a.sg * es % 16 == 0 && a.su * es % 16 == 0 && (!a.dy || a.sdy * es % 16 == 0);
    a.cols = flat ? rows * cols : cols;
    return {flat ? 1 : rows, vec};
}

// <DT, VEC> of a served launch: f(Const<DT>, Const<VEC>) -> the launch's status; UNSUPPORTED where the grid does not hold the tiles
template <class F> int by_swi_kernel(int dtype, SwiGluArgs& a, const SwiWalk& w, F&& f) {
    return by_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        auto go = [&](auto v) {
            constexpr int64_t TILE = SwiIO<DT, decltype(v)::value != 0>::TILE;
            const int64_t tpr = (a.cols + TILE - 1) / TILE;
            if (tpr > 0x7FFFFFFF / w.rows)
                return fail(FQ_ERR_UNSUPPORTED, "%lld rows of %lld columns exceed one launch's grid", (long long)w.rows, (long long)a.cols);
            a.tpr = (uint32_t)tpr;
            begin_launches();
            f(dt, v, dim3((unsigned)(w.rows * tpr)));
            return launch_result();
        };
        return w.vec ? go(Const<1>{}) : go(Const<0>{});
    });
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqa_swiglu_fwd(const void* gate, const void* up, void* y, int64_t rows, int64_t cols, int64_t gate_stride, int64_t up_stride,
                          int dtype, void* stream) {
    if (const int rc = swi_head(rows, cols, {gate_stride, up_stride}, dtype); rc != ROW_CONTINUE) return rc;
    if (!gate || !up || !y) return fail(FQ_ERR_NULL, "gate / up / y must not be NULL");
    if (y == gate || y == up) return fail(FQ_ERR_ARG, "in-place (y == gate or y == up) is not supported");
    SwiGluArgs a{nullptr, gate, up, y, nullptr, cols, 0, gate_stride, up_stride, 0};
    const SwiWalk w = swi_walk(a, rows, cols, dtype, {gate, up, y});
    hipStream_t st = (hipStream_t)stream;
    return by_swi_kernel(dtype, a, w, [&](auto dt, auto v, dim3 grid) {
        launch(swiglu_fwd_kernel<decltype(dt)::value, decltype(v)::value != 0>, grid, dim3(ROW_TPB), st, a);
    });
}

FQ_API int fqa_swiglu_bwd(const void* dy, const void* gate, const void* up, void* dgate, void* dup, int64_t rows, int64_t cols,
                          int64_t dy_stride, int64_t gate_stride, int64_t up_stride, int dtype, void* stream) {
    if (const int rc = swi_head(rows, cols, {dy_stride, gate_stride, up_stride}, dtype); rc != ROW_CONTINUE) return rc;
    if (!dy || !gate || !up) return fail(FQ_ERR_NULL, "dy / gate / up must not be NULL");
    if (!dgate && !dup) return fail(FQ_ERR_NULL, "dgate and dup must not both be NULL");
    if (dgate && (dgate == dy || dgate == gate || dgate == up)) return fail(FQ_ERR_ARG, "in-place (dgate == dy, gate or up) is not supported");
    if (dup && (dup == dy || dup == gate || dup == up)) return fail(FQ_ERR_ARG, "in-place (dup == dy, gate or up) is not supported");
    if (dgate == dup) return fail(FQ_ERR_ARG, "dgate and dup must not be the same buffer");
    SwiGluArgs a{dy, gate, up, dgate, dup, cols, dy_stride, gate_stride, up_stride, 0};
    const SwiWalk w = swi_walk(a, rows, cols, dtype, {dy, gate, up, dgate, dup});      // (a NULL output counts as aligned)
    hipStream_t st = (hipStream_t)stream;
    return by_swi_kernel(dtype, a, w, [&](auto dt, auto v, dim3 grid) {
        constexpr int DT = decltype(dt)::value;
        constexpr bool VEC = decltype(v)::value != 0;
        if (dgate && dup) launch(swiglu_bwd_kernel<DT, VEC, true, true>, grid, dim3(ROW_TPB), st, a);
        else if (dgate) launch(swiglu_bwd_kernel<DT, VEC, true, false>, grid, dim3(ROW_TPB), st, a);
        else launch(swiglu_bwd_kernel<DT, VEC, false, true>, grid, dim3(ROW_TPB), st, a);
    });
}

}  // extern "C"
