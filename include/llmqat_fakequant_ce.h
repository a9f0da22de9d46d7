/* llmqat_fakequant_ce.h -- the language-model loss entry points of libllmqat_fakequant.so (family prefix fqc_).
 *
 * The five other headers' sets of entry points are recorded and stay as they are; the cross-entropy loss of a causal language model's
 * own forward lives here, in the same library, under a prefix of its own.  Conventions as in llmqat_fakequant.h: device pointers, a HIP
 * stream (NULL: the default stream), no allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message of a refusal through
 * the main header's last-error call.  The dtype codes are the main header's.
 *
 * The loss is  cross_entropy(logits, labels, ignore_index, reduction)  over contiguous [rows, cols] logits and [rows] int64 labels, in
 * fp32 arithmetic whatever the logits' dtype.  With y_r the effective label of row r:
 *
 *   shift = 0:  y_r = labels[r]
 *   shift = 1:  the rows are sequences of seq_len positions (rows % seq_len == 0); the last row of every sequence is ignored and every
 *               other row has y_r = labels[r + 1]: logits[..., :-1, :] against labels[..., 1:] on the unshifted pair, with no copy
 *   valid = {r : y_r != ignore_index},  n = |valid|
 *   lse_r = logsumexp(logits row r)
 *   row_loss_r = lse_r - logits[r, y_r]  for valid rows, 0 for ignored ones
 *   loss = sum_valid row_loss / n  (FQC_REDUCTION_MEAN; NaN when n == 0)  or  sum_valid row_loss  (FQC_REDUCTION_SUM; 0 when n == 0),
 *          summed in float64 in row order, rounded once
 *   grad_logits[r, c] = (grad_loss / n) (exp(logits[r, c] - lse_r) - [c == y_r])  for valid rows (the divisor is 1 for SUM), rounded once
 *          to `dtype`; all-zero bits for ignored rows
 *
 * An ignored row is never read: a NaN or inf there reaches neither the loss nor any gradient.  A label outside [0, cols) that is not
 * ignore_index is compared, never used as an address: its row counts as valid, and its row_loss and gradient row are NaN.
 * Row sums run in a fixed order without atomics: two calls on the same inputs give the same bits.
 */
#ifndef LLMQAT_FAKEQUANT_CE_H
#define LLMQAT_FAKEQUANT_CE_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FQC_REDUCTION_MEAN 0
#define FQC_REDUCTION_SUM 1

/* Forward, two launches (the rows, then the sum over rows and the count of valid rows).
 *
 *   logits      contiguous [rows, cols] of `dtype` (FQ_DTYPE_BF16 / F16 / F32), no alignment requirement: 16-byte loads where the base
 *               pointer is 16-byte aligned and cols * itemsize is a multiple of 16, element loads otherwise
 *   labels      [rows] int64
 *   row_lse     [rows] floats out: logsumexp of each valid row (what the backward reads), 0 for ignored rows; NULL: not written
 *   row_loss    [rows] floats out
 *   loss        [1] float out
 *   n_valid     [1] int64 out, 8-byte aligned: the number of valid rows (what the backward divides by under MEAN)
 *
 * No input is written.  Status, in this order and before any HIP call: FQ_ERR_DTYPE (float64, unknown codes), FQ_ERR_SHAPE (negative
 * or zero rows / cols: a loss has no empty launch; rows * cols overflowing; shift = 1 with a positive seq_len that does not divide
 * rows), FQ_ERR_ARG (shift outside {0, 1}, an unknown reduction, seq_len <= 0), FQ_ERR_NULL (logits, labels, row_loss, loss, n_valid),
 * FQ_ERR_UNSUPPORTED (more rows than one launch's grid holds). */
int fqc_ce_fwd(const void* logits, const int64_t* labels, float* row_lse, float* row_loss, float* loss, void* n_valid, int64_t rows,
               int64_t cols, int64_t seq_len, int shift, int64_t ignore_index, int reduction, int dtype, void* stream);

/* Backward, one launch: grad_logits [rows, cols] of `dtype` from the logits, the labels, the forward's row_lse and n_valid, and the
 * upstream gradient of the scalar loss, grad_loss: ONE float in device memory, read by the kernel as n_valid is (no host
 * synchronisation).  The shape, shift, ignore_index and reduction are the forward's.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE, FQ_ERR_SHAPE, FQ_ERR_ARG (shift, reduction, seq_len), FQ_ERR_NULL (any
 * pointer), FQ_ERR_ARG (grad_logits is logits), FQ_ERR_UNSUPPORTED (more rows than one launch's grid holds). */
int fqc_ce_bwd(const void* logits, const int64_t* labels, const float* row_lse, const void* n_valid, const float* grad_loss,
               void* grad_logits, int64_t rows, int64_t cols, int64_t seq_len, int shift, int64_t ignore_index, int reduction, int dtype,
               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_CE_H */
