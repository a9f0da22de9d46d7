/* llmqat_fakequant_train.h -- the training-side entry points of libllmqat_fakequant.so (family prefix fqt_).
 *
 * The main header's set of entry points is recorded call by call (tests/golden/abi_refusals.json) and stays as it is; what a training
 * step needs beyond it lives here, in the same library, under a prefix of its own.  Conventions as in llmqat_fakequant.h: device
 * pointers, a HIP stream (NULL: the default stream), no allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message of
 * a refusal through the main header's last-error call.  The dtype, format and flag codes are the main header's.
 */
#ifndef LLMQAT_FAKEQUANT_TRAIN_H
#define LLMQAT_FAKEQUANT_TRAIN_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* MX block-scaled fake quantization with the blocks running DOWN the columns: the block of x[rows, cols] (contiguous) is the 32
 * elements (32k .. 32k + 31, c) of one column, the arithmetic per block exactly that of the row-axis forward (amax from the bit
 * patterns, a NaN / Inf in the block makes its 32 outputs NaN, the floor or ceil scale rule, one rounding to the dtype).  y[rows, cols]
 * equals the row-axis forward of the transposed tensor, transposed back, bit for bit.  One pass: every element is read once and
 * written once.  A batch of matrices [B, R, C] with R a multiple of 32 is passed as rows = B * R.
 *
 *   fmt     any of the five FQ_MX_* formats (nothing is packed, so FP6 is served)
 *   dtype   FQ_DTYPE_BF16 / F16 / F32
 *   flags   0 or FQ_MX_FLAG_CEIL; any other bit, FQ_MX_FLAG_ROTATE included: FQ_ERR_ARG
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (float64, unknown codes), FQ_ERR_ARG (unknown fmt, flag bits),
 * FQ_ERR_SHAPE (negative or overflowing shape, rows not a multiple of 32), 0 without a launch for an empty shape, FQ_ERR_NULL,
 * FQ_ERR_ARG (y == x), FQ_ERR_UNSUPPORTED (x / y not 16-byte aligned, cols * element size not a multiple of 16, more tiles than one
 * launch's grid holds). */
int fqt_mx_fwd_cols(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, int flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_TRAIN_H */
