/* llmqat_fakequant_loss.h -- the distillation-loss entry points of libllmqat_fakequant.so (family prefix fql_).
 *
 * The four other headers' sets of entry points are recorded and stay as they are; the loss that a quantization-aware distillation step
 * ends with lives here, in the same library, under a prefix of its own.  Conventions as in llmqat_fakequant.h: device pointers, a HIP
 * stream (NULL: the default stream), no allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message of a refusal through
 * the main header's last-error call.  The dtype codes are the main header's.
 *
 * The loss is  kl_div(log_softmax(student), softmax(teacher), reduction = "batchmean")  over contiguous [rows, cols] logits, softmax
 * along cols, in fp32 arithmetic whatever the logits' dtype:
 *
 *   lse_s = logsumexp(student row), lse_t = logsumexp(teacher row), p_s = exp(s - lse_s), p_t = exp(t - lse_t)
 *   row_loss = sum_v p_t (t - s) - lse_t + lse_s        terms with p_t == 0 contribute 0, also where s is -inf
 *   loss     = sum_rows row_loss / batch                summed in float64 in row order, rounded once
 *   grad_student = (grad_loss / batch) (p_s - p_t)      rounded once to `dtype`
 *
 * Row sums run in a fixed order without atomics: two calls on the same inputs give the same bits.
 */
#ifndef LLMQAT_FAKEQUANT_LOSS_H
#define LLMQAT_FAKEQUANT_LOSS_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward, two launches (the rows, then the sum over rows).
 *
 *   student, teacher  contiguous [rows, cols] of `dtype` (FQ_DTYPE_BF16 / F16 / F32), no alignment requirement: 16-byte loads where
 *                     both base pointers are 16-byte aligned and cols * itemsize is a multiple of 16, element loads otherwise
 *   row_stats         [rows, 2] floats out: lse_s, lse_t of each row (what the backward reads); NULL: not written
 *   row_loss          [rows] floats out
 *   loss              [1] float out
 *   batch             the divisor of "batchmean": the logits' first dimension, not the row count
 *
 * Neither input is written.  Status, in this order and before any HIP call: FQ_ERR_DTYPE (float64, unknown codes), FQ_ERR_SHAPE
 * (negative or zero rows / cols: a loss has no empty launch; rows * cols overflowing), FQ_ERR_ARG (batch <= 0), FQ_ERR_NULL (student,
 * teacher, row_loss, loss), FQ_ERR_UNSUPPORTED (more rows than one launch's grid holds). */
int fql_kd_kl_fwd(const void* student, const void* teacher, float* row_stats, float* row_loss, float* loss, int64_t rows, int64_t cols,
                  int64_t batch, int dtype, void* stream);

/* Backward, one launch: grad_student [rows, cols] of `dtype` from the logits, the forward's row_stats and the upstream gradient of the
 * scalar loss, grad_loss: ONE float in device memory, read by the kernel (no host synchronisation).
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE, FQ_ERR_SHAPE, FQ_ERR_ARG (batch <= 0), FQ_ERR_NULL (any pointer),
 * FQ_ERR_ARG (grad_student is student or teacher), FQ_ERR_UNSUPPORTED (more rows than one launch's grid holds). */
int fql_kd_kl_bwd(const void* student, const void* teacher, const float* row_stats, const float* grad_loss, void* grad_student,
                  int64_t rows, int64_t cols, int64_t batch, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_LOSS_H */
