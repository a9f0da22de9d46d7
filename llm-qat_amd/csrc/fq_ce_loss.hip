// fq_ce_loss.hip -- the language-model loss kernels (fq_ce_loss.h) and their entry points (include/llmqat_fakequant_ce.h): a translation
// unit of its own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_ce.h"

#include "fq_ce_loss.h"

using namespace fq;

namespace {

// what both entry points check first, in the header's order: ROW_CONTINUE, or the refusal.  Every check comes before any HIP call.
int ce_head(int64_t rows, int64_t cols, int64_t seq_len, int shift, int reduction, int dtype) {
    if (const int rc = row_head("loss", rows, cols, {dtype}); rc != ROW_CONTINUE) return rc;
    if (shift == 1 && seq_len > 0 && rows % seq_len != 0)
        return fail(FQ_ERR_SHAPE, "shift=1: rows=%lld is not whole sequences of seq_len=%lld", (long long)rows, (long long)seq_len);
    if (shift != 0 && shift != 1) return fail(FQ_ERR_ARG, "shift=%d must be 0 or 1", shift);
    if (reduction != FQC_REDUCTION_MEAN && reduction != FQC_REDUCTION_SUM)
        return fail(FQ_ERR_ARG, "unknown reduction code %d (FQC_REDUCTION_MEAN and FQC_REDUCTION_SUM are served)", reduction);
    if (seq_len <= 0) return fail(FQ_ERR_ARG, "seq_len=%lld must be positive", (long long)seq_len);
    return ROW_CONTINUE;
}

template <int DT> int launch_ce_fwd(bool vec, CeFwdArgs a, float* loss, int64_t* n_valid, int reduction, hipStream_t st) {
    begin_launches();
    by_row_shape(a.cols, vec, [&](auto v, auto tpr) {
        launch_rows<decltype(tpr)::value>(ce_fwd_kernel<DT, decltype(v)::value != 0, decltype(tpr)::value>, a.lab.rows, st, a);
    });
    launch(ce_sum_kernel, dim3(1), dim3(CE_SUM_TPB), st, (const float*)a.row_loss, a.lab, loss, n_valid, reduction);
    return launch_result();
}

template <int DT> int launch_ce_bwd(bool vec, CeBwdArgs a, hipStream_t st) {
    begin_launches();
    by_row_shape(a.cols, vec, [&](auto v, auto tpr) {
        launch_rows<decltype(tpr)::value>(ce_bwd_kernel<DT, decltype(v)::value != 0, decltype(tpr)::value>, a.lab.rows, st, a);
    });
    return launch_result();
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqc_ce_fwd(const void* logits, const int64_t* labels, float* row_lse, float* row_loss, float* loss, void* n_valid, int64_t rows,
                      int64_t cols, int64_t seq_len, int shift, int64_t ignore_index, int reduction, int dtype, void* stream) {
    if (const int rc = ce_head(rows, cols, seq_len, shift, reduction, dtype); rc != ROW_CONTINUE) return rc;
    if (!logits || !labels || !row_loss || !loss || !n_valid) return fail(FQ_ERR_NULL, "logits / labels / row_loss / loss / n_valid must not be NULL");
    if (const int rc = row_grid_check(rows, cols); rc != ROW_CONTINUE) return rc;
    const CeFwdArgs a{logits, CeLabels{labels, rows, seq_len, ignore_index, shift}, row_lse, row_loss, cols};
    const bool vec = row_vec(cols, dtype, logits);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_ce_fwd<decltype(dt)::value>(vec, a, loss, (int64_t*)n_valid, reduction, st); });
}

FQ_API int fqc_ce_bwd(const void* logits, const int64_t* labels, const float* row_lse, const void* n_valid, const float* grad_loss,
                      void* grad_logits, int64_t rows, int64_t cols, int64_t seq_len, int shift, int64_t ignore_index, int reduction,
                      int dtype, void* stream) {
    if (const int rc = ce_head(rows, cols, seq_len, shift, reduction, dtype); rc != ROW_CONTINUE) return rc;
    if (!logits || !labels || !row_lse || !n_valid || !grad_loss || !grad_logits)
        return fail(FQ_ERR_NULL, "logits / labels / row_lse / n_valid / grad_loss / grad_logits must not be NULL");
    if (grad_logits == logits) return fail(FQ_ERR_ARG, "in-place (grad_logits == logits) is not supported");
    if (const int rc = row_grid_check(rows, cols); rc != ROW_CONTINUE) return rc;
    const CeBwdArgs a{logits, CeLabels{labels, rows, seq_len, ignore_index, shift}, row_lse, (const int64_t*)n_valid, grad_loss, grad_logits,
                      cols, reduction};
    const bool vec = row_vec(cols, dtype, logits, grad_logits);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_ce_bwd<decltype(dt)::value>(vec, a, st); });
}

}  // extern "C"
