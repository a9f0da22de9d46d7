// fq_ce_loss.hip -- the language-model loss kernels (fq_ce_loss.h) and their entry points (include/llmqat_fakequant_ce.h): a translation
// unit of its own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_ce.h"

#include "fq_ce_loss.h"

using namespace fq;

namespace {

constexpr int CONTINUE = 1;

// what both entry points check first, in the header's order: CONTINUE, or the refusal.  Every check comes before any HIP call.
int ce_head(int64_t rows, int64_t cols, int64_t seq_len, int shift, int reduction, int dtype) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the loss entry points");
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (rows == 0 || cols == 0) return fail(FQ_ERR_SHAPE, "empty shape rows=%lld cols=%lld: a loss has no empty launch", (long long)rows, (long long)cols);
    if (rows > INT64_MAX / 4 / cols) return fail(FQ_ERR_SHAPE, "rows * cols overflows");
    if (shift == 1 && seq_len > 0 && rows % seq_len != 0)
        return fail(FQ_ERR_SHAPE, "shift=1: rows=%lld is not whole sequences of seq_len=%lld", (long long)rows, (long long)seq_len);
    if (shift != 0 && shift != 1) return fail(FQ_ERR_ARG, "shift=%d must be 0 or 1", shift);
    if (reduction != FQC_REDUCTION_MEAN && reduction != FQC_REDUCTION_SUM)
        return fail(FQ_ERR_ARG, "unknown reduction code %d (FQC_REDUCTION_MEAN and FQC_REDUCTION_SUM are served)", reduction);
    if (seq_len <= 0) return fail(FQ_ERR_ARG, "seq_len=%lld must be positive", (long long)seq_len);
    return CONTINUE;
}

// rows of CE_WIDE elements or more: a workgroup each; shorter ones: a wave each, four to a workgroup
bool ce_wide(int64_t cols) { return cols >= CE_WIDE; }
int64_t ce_grid(int64_t rows, int64_t cols) { return ce_wide(cols) ? rows : (rows + 3) / 4; }
int ce_grid_check(int64_t rows, int64_t cols) {
    if (ce_grid(rows, cols) > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "%lld rows exceed one launch's grid", (long long)rows);
    return CONTINUE;
}
// 16-byte accesses: every row of every tensor starts on a 16-byte boundary and is whole vectors
bool ce_vec(int64_t cols, int dtype, const void* p0, const void* p1 = nullptr) {
    return aligned16(p0) && aligned16(p1) && cols * esize_of(dtype) % 16 == 0;
}

template <int DT> int launch_ce_fwd(bool vec, CeFwdArgs a, float* loss, int64_t* n_valid, int reduction, hipStream_t st) {
    begin_launches();
    const dim3 grid((unsigned)ce_grid(a.lab.rows, a.cols)), block(KD_TPB);
    if (ce_wide(a.cols)) {
        if (vec) launch(ce_fwd_kernel<DT, true, 256>, grid, block, st, a);
        else launch(ce_fwd_kernel<DT, false, 256>, grid, block, st, a);
    } else {
        if (vec) launch(ce_fwd_kernel<DT, true, 64>, grid, block, st, a);
        else launch(ce_fwd_kernel<DT, false, 64>, grid, block, st, a);
    }
    launch(ce_sum_kernel, dim3(1), dim3(CE_SUM_TPB), st, (const float*)a.row_loss, a.lab, loss, n_valid, reduction);
    return launch_result();
}

template <int DT> int launch_ce_bwd(bool vec, CeBwdArgs a, hipStream_t st) {
    begin_launches();
    const dim3 grid((unsigned)ce_grid(a.lab.rows, a.cols)), block(KD_TPB);
    if (ce_wide(a.cols)) {
        if (vec) launch(ce_bwd_kernel<DT, true, 256>, grid, block, st, a);
        else launch(ce_bwd_kernel<DT, false, 256>, grid, block, st, a);
    } else {
        if (vec) launch(ce_bwd_kernel<DT, true, 64>, grid, block, st, a);
        else launch(ce_bwd_kernel<DT, false, 64>, grid, block, st, a);
    }
    return launch_result();
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqc_ce_fwd(const void* logits, const int64_t* labels, float* row_lse, float* row_loss, float* loss, void* n_valid, int64_t rows,
                      int64_t cols, int64_t seq_len, int shift, int64_t ignore_index, int reduction, int dtype, void* stream) {
    if (const int rc = ce_head(rows, cols, seq_len, shift, reduction, dtype); rc != CONTINUE) return rc;
    if (!logits || !labels || !row_loss || !loss || !n_valid) return fail(FQ_ERR_NULL, "logits / labels / row_loss / loss / n_valid must not be NULL");
    if (const int rc = ce_grid_check(rows, cols); rc != CONTINUE) return rc;
    const CeFwdArgs a{logits, CeLabels{labels, rows, seq_len, ignore_index, shift}, row_lse, row_loss, cols};
    const bool vec = ce_vec(cols, dtype, logits);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_ce_fwd<decltype(dt)::value>(vec, a, loss, (int64_t*)n_valid, reduction, st); });
}

FQ_API int fqc_ce_bwd(const void* logits, const int64_t* labels, const float* row_lse, const void* n_valid, const float* grad_loss,
                      void* grad_logits, int64_t rows, int64_t cols, int64_t seq_len, int shift, int64_t ignore_index, int reduction,
                      int dtype, void* stream) {
    if (const int rc = ce_head(rows, cols, seq_len, shift, reduction, dtype); rc != CONTINUE) return rc;
    if (!logits || !labels || !row_lse || !n_valid || !grad_loss || !grad_logits)
        return fail(FQ_ERR_NULL, "logits / labels / row_lse / n_valid / grad_loss / grad_logits must not be NULL");
    if (grad_logits == logits) return fail(FQ_ERR_ARG, "in-place (grad_logits == logits) is not supported");
    if (const int rc = ce_grid_check(rows, cols); rc != CONTINUE) return rc;
    const CeBwdArgs a{logits, CeLabels{labels, rows, seq_len, ignore_index, shift}, row_lse, (const int64_t*)n_valid, grad_loss, grad_logits,
                      cols, reduction};
    const bool vec = ce_vec(cols, dtype, logits, grad_logits);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_ce_bwd<decltype(dt)::value>(vec, a, st); });
}

}  // extern "C"
