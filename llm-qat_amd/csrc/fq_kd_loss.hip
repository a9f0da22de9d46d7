// fq_kd_loss.hip -- the distillation-loss kernels (fq_kd_loss.h) and their entry points (include/llmqat_fakequant_loss.h): a translation
// unit of its own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_loss.h"

#include "fq_kd_loss.h"

using namespace fq;

namespace {

constexpr int CONTINUE = 1;

// what both entry points check first, in the header's order: CONTINUE, or the refusal.  Every check comes before any HIP call.
int kd_head(int64_t rows, int64_t cols, int64_t batch, int dtype) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the loss entry points");
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return fail(FQ_ERR_SHAPE, "empty shape rows=%lld cols=%lld: a loss has no empty launch", (long long)rows, (long long)cols);
    if (rows > INT64_MAX / 4 / cols) return fail(FQ_ERR_SHAPE, "rows * cols overflows");
    if (batch <= 0) return fail(FQ_ERR_ARG, "batch=%lld must be positive", (long long)batch);
    return CONTINUE;
}

// rows of KD_WIDE elements or more: a workgroup each; shorter ones: a wave each, four to a workgroup
bool kd_wide(int64_t cols) { return cols >= KD_WIDE; }
int64_t kd_grid(int64_t rows, int64_t cols) { return kd_wide(cols) ? rows : (rows + 3) / 4; }
int kd_grid_check(int64_t rows, int64_t cols) {
    if (kd_grid(rows, cols) > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "%lld rows exceed one launch's grid", (long long)rows);
    return CONTINUE;
}
// 16-byte accesses: every row of every tensor starts on a 16-byte boundary and is whole vectors
bool kd_vec(int64_t cols, int dtype, const void* p0, const void* p1, const void* p2 = nullptr) {
    return aligned16(p0) && aligned16(p1) && aligned16(p2) && cols * esize_of(dtype) % 16 == 0;
}

template <int DT> int launch_kd_fwd(bool vec, KdFwdArgs a, float* loss, int64_t batch, hipStream_t st) {
    begin_launches();
    const dim3 grid((unsigned)kd_grid(a.rows, a.cols)), block(KD_TPB);
    if (kd_wide(a.cols)) {
        if (vec) launch(kd_fwd_kernel<DT, true, 256>, grid, block, st, a);
        else launch(kd_fwd_kernel<DT, false, 256>, grid, block, st, a);
    } else {
        if (vec) launch(kd_fwd_kernel<DT, true, 64>, grid, block, st, a);
        else launch(kd_fwd_kernel<DT, false, 64>, grid, block, st, a);
    }
    launch(kd_sum_kernel, dim3(1), block, st, (const float*)a.row_loss, loss, a.rows, (double)batch);
    return launch_result();
}

template <int DT> int launch_kd_bwd(bool vec, KdBwdArgs a, hipStream_t st) {
    begin_launches();
    const dim3 grid((unsigned)kd_grid(a.rows, a.cols)), block(KD_TPB);
    if (kd_wide(a.cols)) {
        if (vec) launch(kd_bwd_kernel<DT, true, 256>, grid, block, st, a);
        else launch(kd_bwd_kernel<DT, false, 256>, grid, block, st, a);
    } else {
        if (vec) launch(kd_bwd_kernel<DT, true, 64>, grid, block, st, a);
        else launch(kd_bwd_kernel<DT, false, 64>, grid, block, st, a);
    }
    return launch_result();
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fql_kd_kl_fwd(const void* student, const void* teacher, float* row_stats, float* row_loss, float* loss, int64_t rows, int64_t cols,
                         int64_t batch, int dtype, void* stream) {
    if (const int rc = kd_head(rows, cols, batch, dtype); rc != CONTINUE) return rc;
    if (!student || !teacher || !row_loss || !loss) return fail(FQ_ERR_NULL, "student / teacher / row_loss / loss must not be NULL");
    if (const int rc = kd_grid_check(rows, cols); rc != CONTINUE) return rc;
    const KdFwdArgs a{student, teacher, row_stats, row_loss, rows, cols};
    const bool vec = kd_vec(cols, dtype, student, teacher);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_kd_fwd<decltype(dt)::value>(vec, a, loss, batch, st); });
}

FQ_API int fql_kd_kl_bwd(const void* student, const void* teacher, const float* row_stats, const float* grad_loss, void* grad_student,
                         int64_t rows, int64_t cols, int64_t batch, int dtype, void* stream) {
    if (const int rc = kd_head(rows, cols, batch, dtype); rc != CONTINUE) return rc;
    if (!student || !teacher || !row_stats || !grad_loss || !grad_student)
        return fail(FQ_ERR_NULL, "student / teacher / row_stats / grad_loss / grad_student must not be NULL");
    if (grad_student == student || grad_student == teacher) return fail(FQ_ERR_ARG, "in-place (grad_student == student or teacher) is not supported");
    if (const int rc = kd_grid_check(rows, cols); rc != CONTINUE) return rc;
    const KdBwdArgs a{student, teacher, row_stats, grad_loss, grad_student, rows, cols, (float)batch};
    const bool vec = kd_vec(cols, dtype, student, teacher, grad_student);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_kd_bwd<decltype(dt)::value>(vec, a, st); });
}

}  // extern "C"
