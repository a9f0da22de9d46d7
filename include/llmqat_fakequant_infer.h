/* llmqat_fakequant_infer.h -- the inference-side entry points of libllmqat_fakequant.so (family prefix fqi_).
 *
 * The main header's set of entry points, the training header's and the stochastic-rounding header's are recorded and stay as they are;
 * what serving a trained model needs beyond them lives here, in the same library, under a prefix of its own.  Conventions as in
 * llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default stream), no allocation, no synchronisation, 0 or a negative
 * FQ_ERR_* code, the message of a refusal through the main header's last-error call.  The dtype and format codes are the main header's.
 */
#ifndef LLMQAT_FAKEQUANT_INFER_H
#define LLMQAT_FAKEQUANT_INFER_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An MX export back to a tensor, one launch: y[rows, cols] (contiguous, `dtype`) from the element codes and the E8M0 scale bytes that
 * the main header's export entry points write for a contiguous [rows, cols] tensor.
 *
 *   elems   rows * cols / 2 bytes for FQ_MX_FP4_E2M1 (element 2k in the low nibble of byte k, bit 3 of a code its sign), rows * cols
 *           bytes for FQ_MX_FP8_E4M3 / FQ_MX_FP8_E5M2 (the float8_e4m3fn / float8_e5m2 bit patterns, their NaN / Inf codes included)
 *   scales  rows * cols / 32 bytes, one per block of 32 consecutive elements: 2^(byte - 127); byte 0 is 2^-127; byte 0xFF makes the
 *           block's 32 outputs NaN
 *   y       value of the code * scale, computed in fp32 (exact, or +-Inf; fp32 subnormals are kept) and rounded once, nearest-even, to
 *           `dtype` (FQ_DTYPE_BF16 / F16 / F32), with gradual underflow in its subnormal range; -0 stays -0
 *
 * Neither input is written.  Status, in this order and before any HIP call: FQ_ERR_DTYPE (float64, unknown codes), FQ_ERR_ARG (unknown
 * fmt), FQ_ERR_ARG (an FP6 format: it has no export packing), FQ_ERR_SHAPE (negative or overflowing shape, cols not a multiple of 32),
 * 0 without a launch for an empty shape, FQ_ERR_NULL, FQ_ERR_UNSUPPORTED (elems or y not 16-byte aligned, more vectors than one
 * launch's grid holds). */
int fqi_mx_dequant(const void* elems, const void* scales, void* y, int64_t rows, int64_t cols, int fmt, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_INFER_H */
