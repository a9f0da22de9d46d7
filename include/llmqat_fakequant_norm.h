/* llmqat_fakequant_norm.h -- the RMSNorm entry points of libllmqat_fakequant.so (family prefix fqn_).
 *
 * The six other headers' sets of entry points are recorded and stay as they are; the root-mean-square layer norm that stands in front of
 * every quantized projection of a LLaMA decoder layer lives here, in the same library, under a prefix of its own.  Conventions as in
 * llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default stream), no allocation, no synchronisation, 0 or a negative
 * FQ_ERR_* code, the message of a refusal through the main header's last-error call.  The dtype codes are the main header's.
 *
 * x is contiguous [rows, cols] of x_dtype, w is [cols] of w_dtype, y and g = dL/dy are [rows, cols] of w_dtype, dx has x_dtype and dw
 * has w_dtype.  Served (x_dtype, w_dtype) pairs: equal dtypes (F32, BF16, F16) and every pair in which exactly
 * one of the two is F32: seven pairs.  float64 and the BF16-with-F16 pairs are refused.  The arithmetic is fp32 for all of them:
 *
 *   forward    ss_r   = sum_c x[r,c]^2                  fp32, a fixed summation order, no rescaling (a sum that overflows gives rstd = 0)
 *              rstd_r = rsqrt(ss_r / cols + eps)
 *              n[r,c] = x[r,c] * rstd_r                 one fp32 rounding
 *              w 16-bit:  y = rb(w[c] * rb(n[r,c]))     rb: round to w_dtype (nearest even) and back
 *              w fp32:    y = w[c] * n[r,c]
 *   backward   a[r,c]  = g[r,c] * w[c],   n = x * rstd (not rounded)
 *              s_r     = (sum_c a[r,c] n[r,c]) / cols
 *              dx[r,c] = rstd_r (a[r,c] - n[r,c] s_r)   rounded once to x_dtype
 *              dw[c]   = sum_r g[r,c] n[r,c]            fp32, a fixed order, rounded once to w_dtype
 *                        the fixed order: within a part its rows in row order; then, per column, the parts' partial sums as 16 runs of
 *                        ceil(parts / 16) consecutive parts, each run summed in index order, and the 16 runs added in index order
 *                        (not one pass over the parts in index order: that is a chain of `parts` dependent additions per column)
 *
 * No atomics anywhere: two calls on the same inputs give the same bits.  No alignment requirement: 16-byte loads and stores where the
 * dtypes are equal, every base pointer is 16-byte aligned and cols * itemsize is a multiple of 16; element accesses that feed the same
 * arithmetic otherwise.
 */
#ifndef LLMQAT_FAKEQUANT_NORM_H
#define LLMQAT_FAKEQUANT_NORM_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward, one launch.  rstd: [rows] floats out, what the backward reads; NULL: not written.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (unknown codes, float64, a pair that is not served), FQ_ERR_SHAPE
 * (negative or zero rows / cols; rows * cols overflowing), FQ_ERR_ARG (eps negative, NaN or inf), FQ_ERR_NULL (x, w, y), FQ_ERR_ARG
 * (y is x or w), FQ_ERR_UNSUPPORTED (more rows than one launch's grid holds). */
int fqn_rms_norm_fwd(const void* x, const void* w, void* y, float* rstd, int64_t rows, int64_t cols, float eps, int x_dtype, int w_dtype,
                     void* stream);

/* The backward's row chunks: launch 1 gives each of `parts` workgroups (rows of fewer than 2048 elements: waves) a run of
 * ceil(rows / parts) consecutive rows, and writes one fp32 partial sum of g n per part and column.  Pure functions of the shape; 0 for a
 * shape the entry points refuse with FQ_ERR_SHAPE (negative, empty, rows * cols overflowing).  A shape they refuse only with
 * FQ_ERR_UNSUPPORTED (a grid that one launch does not hold) still has its parts and its byte count. */
int64_t fqn_rms_norm_bwd_parts(int64_t rows, int64_t cols);
/* parts * cols * 4: the bytes of the fp32 [parts, cols] partial-sum buffer the caller owns (16-byte aligned for the 16-byte path) */
size_t fqn_rms_norm_bwd_workspace_bytes(int64_t rows, int64_t cols);

/* Backward, two launches: the rows (dx, and the parts' partial sums), then the sum over the parts (dw).  dx NULL: not stored.  dw NULL:
 * the partial sums are not written, the second launch is skipped and the workspace is not looked at.  Not both may be NULL.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE, FQ_ERR_SHAPE, FQ_ERR_NULL (g, x, w, rstd; dx and dw both; the workspace
 * where dw is wanted), FQ_ERR_ARG (dx is g, x or w; dw is g, x or w), FQ_ERR_WORKSPACE (fewer than fqn_rms_norm_bwd_workspace_bytes),
 * FQ_ERR_UNSUPPORTED (dw wanted for more columns than the second launch's grid holds; more parts than the first launch's grid holds). */
int fqn_rms_norm_bwd(const void* g, const void* x, const void* w, const float* rstd, void* dx, void* dw, void* workspace,
                     size_t workspace_bytes, int64_t rows, int64_t cols, int x_dtype, int w_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_NORM_H */
