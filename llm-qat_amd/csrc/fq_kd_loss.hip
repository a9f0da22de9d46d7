// fq_kd_loss.hip -- the distillation-loss kernels (fq_kd_loss.h) and their entry points (include/llmqat_fakequant_loss.h): a translation
// unit of its own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_loss.h"

#include "fq_kd_loss.h"

using namespace fq;

namespace {

// what both entry points check first, in the header's order: ROW_CONTINUE, or the refusal.  Every check comes before any HIP call.
int kd_head(int64_t rows, int64_t cols, int64_t batch, int dtype) {
    if (const int rc = row_head("loss", rows, cols, {dtype}); rc != ROW_CONTINUE) return rc;
    if (batch <= 0) return fail(FQ_ERR_ARG, "batch=%lld must be positive", (long long)batch);
    return ROW_CONTINUE;
}

template <int DT> int launch_kd_fwd(bool vec, KdFwdArgs a, float* loss, int64_t batch, hipStream_t st) {
    begin_launches();
    by_row_shape(a.cols, vec, [&](auto v, auto tpr) {
        launch_rows<decltype(tpr)::value>(kd_fwd_kernel<DT, decltype(v)::value != 0, decltype(tpr)::value>, a.rows, st, a);
    });
    launch(kd_sum_kernel, dim3(1), dim3(KD_SUM_TPB), st, (const float*)a.row_loss, loss, a.rows, (double)batch);
    return launch_result();
}

template <int DT> int launch_kd_bwd(bool vec, KdBwdArgs a, hipStream_t st) {
    begin_launches();
    by_row_shape(a.cols, vec, [&](auto v, auto tpr) {
        launch_rows<decltype(tpr)::value>(kd_bwd_kernel<DT, decltype(v)::value != 0, decltype(tpr)::value>, a.rows, st, a);
    });
    return launch_result();
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fql_kd_kl_fwd(const void* student, const void* teacher, float* row_stats, float* row_loss, float* loss, int64_t rows, int64_t cols,
                         int64_t batch, int dtype, void* stream) {
    if (const int rc = kd_head(rows, cols, batch, dtype); rc != ROW_CONTINUE) return rc;
    if (!student || !teacher || !row_loss || !loss) return fail(FQ_ERR_NULL, "student / teacher / row_loss / loss must not be NULL");
    if (const int rc = row_grid_check(rows, cols); rc != ROW_CONTINUE) return rc;
    const KdFwdArgs a{student, teacher, row_stats, row_loss, rows, cols};
    const bool vec = row_vec(cols, dtype, student, teacher);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_kd_fwd<decltype(dt)::value>(vec, a, loss, batch, st); });
}

FQ_API int fql_kd_kl_bwd(const void* student, const void* teacher, const float* row_stats, const float* grad_loss, void* grad_student,
                         int64_t rows, int64_t cols, int64_t batch, int dtype, void* stream) {
    if (const int rc = kd_head(rows, cols, batch, dtype); rc != ROW_CONTINUE) return rc;
    if (!student || !teacher || !row_stats || !grad_loss || !grad_student)
        return fail(FQ_ERR_NULL, "student / teacher / row_stats / grad_loss / grad_student must not be NULL");
    if (grad_student == student || grad_student == teacher) return fail(FQ_ERR_ARG, "in-place (grad_student == student or teacher) is not supported");
    if (const int rc = row_grid_check(rows, cols); rc != ROW_CONTINUE) return rc;
    const KdBwdArgs a{student, teacher, row_stats, grad_loss, grad_student, rows, cols, (float)batch};
    const bool vec = row_vec(cols, dtype, student, teacher, grad_student);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_kd_bwd<decltype(dt)::value>(vec, a, st); });
}

}  // extern "C"
