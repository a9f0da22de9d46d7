// fq_rms_norm.hip -- the RMSNorm kernels (fq_rms_norm.h) and their entry points (include/llmqat_fakequant_norm.h): a translation unit of
// its own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_norm.h"

#include <cmath>

#include "fq_rms_norm.h"

using namespace fq;

namespace {

// what both entry points check first, in the header's order: ROW_CONTINUE, or the refusal.  Every check comes before any HIP call.
int rms_head(int64_t rows, int64_t cols, int x_dtype, int w_dtype) {
    return row_head("norm", rows, cols, {x_dtype, w_dtype}, [&] {
        if (x_dtype == w_dtype || x_dtype == FQ_DTYPE_F32 || w_dtype == FQ_DTYPE_F32) return ROW_CONTINUE;
        return fail(FQ_ERR_DTYPE, "the dtype pair (x %d, w %d) is not served: equal dtypes, or one of the two float32", x_dtype, w_dtype);
    });
}
// the size queries' question, "is this shape served": the shape's checks alone, and no message
bool rms_shape_served(int64_t rows, int64_t cols) { return row_head(nullptr, rows, cols) == ROW_CONTINUE; }

// the kernel <XDT, WDT, VEC, TPR, NGV> of a served pair: f(Const<XDT>, Const<WDT>, Const<VEC>, Const<TPR>, Const<NGV>).  The 16-byte path
// exists for equal dtypes, built for a quarter, a half and all of the most vectors a lane holds: the smallest that holds the row (a
// function of cols alone, so the summation order is one too); the element path has one form (NGV = 0)
template <class F> int by_rms_kernel(int x_dtype, int w_dtype, int64_t cols, bool vec, F&& f) {
    return by_dtype(x_dtype, [&](auto xd) {
        return by_dtype(w_dtype, [&](auto wd) {
            constexpr int XDT = decltype(xd)::value, WDT = decltype(wd)::value;
            if constexpr (XDT == WDT || XDT == F32 || WDT == F32) {
                by_row_shape(cols, vec, [&](auto v, auto tpr) {
                    constexpr int V = decltype(v)::value, TPR = decltype(tpr)::value;
                    if constexpr (V == 0) {
                        f(Const<XDT>{}, Const<WDT>{}, Const<0>{}, Const<TPR>{}, Const<0>{});
                    } else if constexpr (XDT == WDT) {
                        constexpr int MOST = rms_most_groups<XDT>();
                        const int64_t need = (cols * Ty<XDT>::ESIZE / 16 + TPR - 1) / TPR;      // vectors of a lane
                        if (need <= rms_groups(MOST, 2)) f(Const<XDT>{}, Const<WDT>{}, Const<1>{}, Const<TPR>{}, Const<rms_groups(MOST, 2)>{});
                        else if (need <= rms_groups(MOST, 1)) f(Const<XDT>{}, Const<WDT>{}, Const<1>{}, Const<TPR>{}, Const<rms_groups(MOST, 1)>{});
                        else f(Const<XDT>{}, Const<WDT>{}, Const<1>{}, Const<TPR>{}, Const<MOST>{});
                    }
                });
                return launch_result();
            } else {
                return fail(FQ_ERR_DTYPE, "the dtype pair is not served");
            }
        });
    });
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqn_rms_norm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int64_t cols, float eps, int x_dtype,
                            int w_dtype, void* stream) {
    if (const int rc = rms_head(rows, cols, x_dtype, w_dtype); rc != ROW_CONTINUE) return rc;
    if (!(eps >= 0.0f) || std::isinf(eps)) return fail(FQ_ERR_ARG, "eps=%g must be finite and not negative", (double)eps);
    if (!x || !w || !y) return fail(FQ_ERR_NULL, "x / w / y must not be NULL");
    if (y == x || y == w) return fail(FQ_ERR_ARG, "in-place (y == x or y == w) is not supported");
    if (const int rc = row_grid_check(rows, cols); rc != ROW_CONTINUE) return rc;
    const RmsFwdArgs a{x, w, y, rstd, rows, cols, eps};
    const bool vec = x_dtype == w_dtype && row_vec(cols, x_dtype, x, w, y);
    hipStream_t st = (hipStream_t)stream;
    begin_launches();
    return by_rms_kernel(x_dtype, w_dtype, cols, vec, [&](auto xd, auto wd, auto v, auto tpr, auto ng) {
        launch_rows<decltype(tpr)::value>(rms_fwd_kernel<decltype(xd)::value, decltype(wd)::value, decltype(v)::value != 0, decltype(tpr)::value, decltype(ng)::value>,
                                          rows, st, a);
    });
}

FQ_API int64_t fqn_rms_norm_bwd_parts(int64_t rows, int64_t cols) { return rms_shape_served(rows, cols) ? rms_parts(rows, cols) : 0; }

FQ_API size_t fqn_rms_norm_bwd_workspace_bytes(int64_t rows, int64_t cols) {
    return rms_shape_served(rows, cols) ? (size_t)rms_parts(rows, cols) * (size_t)cols * sizeof(float) : 0;
}

FQ_API int fqn_rms_norm_bwd(const void* g, const void* x, const void* w, const float* rstd, void* dx, void* dw, void* workspace,
                            size_t workspace_bytes, int64_t rows, int64_t cols, int x_dtype, int w_dtype, void* stream) {
    if (const int rc = rms_head(rows, cols, x_dtype, w_dtype); rc != ROW_CONTINUE) return rc;
    if (!g || !x || !w || !rstd) return fail(FQ_ERR_NULL, "g / x / w / rstd must not be NULL");
    if (!dx && !dw) return fail(FQ_ERR_NULL, "dx and dw must not both be NULL");
    if (dw && !workspace) return fail(FQ_ERR_NULL, "the workspace must not be NULL where dw is wanted");
    if (dx && (dx == g || dx == x || dx == w)) return fail(FQ_ERR_ARG, "in-place (dx == g, x or w) is not supported");
    if (dw && (dw == g || dw == x || dw == w)) return fail(FQ_ERR_ARG, "in-place (dw == g, x or w) is not supported");
    const int64_t parts = rms_parts(rows, cols);
    if (dw && workspace_bytes < (size_t)parts * (size_t)cols * sizeof(float))
        return fail(FQ_ERR_WORKSPACE, "workspace too small: need %zu bytes", (size_t)parts * (size_t)cols * sizeof(float));
    const int64_t dw_grid = (cols + RMS_DW_COLS - 1) / RMS_DW_COLS;
    if (dw && dw_grid > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "%lld columns exceed one launch's grid", (long long)cols);
    if (const int rc = row_grid_check(parts, cols); rc != ROW_CONTINUE) return rc;
    float* ws = dw ? (float*)workspace : nullptr;
    const RmsBwdArgs a{g, x, w, rstd, dx, ws, rows, cols, parts, rms_rows_per_part(rows, cols)};
    const bool vec = x_dtype == w_dtype && row_vec(cols, x_dtype, g, x, w) && aligned16(dx) && aligned16(ws);
    hipStream_t st = (hipStream_t)stream;
    begin_launches();
    const int rc = by_rms_kernel(x_dtype, w_dtype, cols, vec, [&](auto xd, auto wd, auto v, auto tpr, auto ng) {
        launch_rows<decltype(tpr)::value>(rms_bwd_kernel<decltype(xd)::value, decltype(wd)::value, decltype(v)::value != 0, decltype(tpr)::value, decltype(ng)::value>,
                                          parts, st, a);
    });
    if (rc != FQ_OK || !dw) return rc;
    return by_dtype(w_dtype, [&](auto wd) {
        launch(rms_dw_kernel<decltype(wd)::value>, dim3((unsigned)dw_grid), dim3(RMS_DW_TPB), st, (const float*)ws, dw, parts, cols);
        return launch_result();
    });
}

}  // extern "C"
