/* llmqat_fakequant_attn.h -- the attention-softmax entry points of libllmqat_fakequant.so (family prefix fqs2_).
 *
 * The nine other headers' sets of entry points are recorded and stay as they are; the chain that every decoder layer runs between its two
 * attention products (the reference's models/modeling_llama_quant.py:352-375: the division by sqrt(head_dim), the additive mask, the
 * clamp at finfo.min and the fp32 softmax with its cast back) lives here, in the same library, under a prefix of its own.  Conventions as
 * in llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default stream), no allocation, no synchronisation, 0 or a negative
 * FQ_ERR_* code, the message of a refusal through the main header's last-error call.  The dtype codes are the main header's.  No atomics
 * and no workspace: two calls on the same inputs give the same bits.
 *
 * Tensors.  scores is [rows, cols] contiguous, rows = B * H * T (the [B, H, T, S] product with cols = S), dtype ds: F32, BF16 or F16;
 * float64 is refused.  mask is NULL or [B, 1, T, S], given as a base pointer, a batch stride and a row stride in elements (not negative;
 * the batch stride may be 0, an expanded mask), last stride 1; its dtype dm is ds or F32 (mask_dtype is not looked at where mask is NULL).
 * y is [rows, cols] of ds.  stats is fp32 [rows, 2], the row's maximum and its sum of exponentials, or NULL: not written.  All index
 * arithmetic is 64-bit.
 *
 * Arithmetic: fp32 with the chain's roundings up to the softmax.  P = ds where dm is ds or the mask is NULL, else F32 (the sum promotes);
 * rb_X rounds to dtype X (nearest even) and back; MIN_P = the most negative finite value of P; x a score, m its mask element:
 *
 *   a = rb_P( rb_ds(x * inv) + m )             without a mask: a = rb_ds(x * inv), and z = a (the reference clamps under a mask only)
 *   z = a < MIN_P ? MIN_P : a                  -inf becomes MIN_P, NaN stays NaN
 *   p = exp(z - max_row z) / sum_row exp(z - max_row z)
 *   y = rb_ds(p)
 *
 * inv is the caller's fp32 reciprocal of (float)sqrt(head_dim): tensor / python_float on the device is a product with that reciprocal.
 *
 * Backward, from g = dL/dy (dtype ds), the scores, the mask and the forward's stats: p is recomputed (the forward's fp32 p bit for bit),
 * dot = sum_row g p in a fixed order, and
 *
 *   d  = rb_P( (g - dot) p )
 *   d  = a > MIN_P ? d : (a == MIN_P ? rb_P(d / 2) : 0)        a NaN: d passes; no mask: d passes (the gradient of torch.max, ties halved)
 *   dx = rb_ds( rb_ds(d) * inv )
 *
 * A NaN or +inf in a row makes the row NaN, as in ATen; other rows are not touched.
 *
 * No alignment requirement: 16-byte loads and stores where every base pointer and the mask's strides in bytes are 16-byte aligned and
 * cols * itemsize(ds) is a multiple of 16 (the mixed pairs, 16-bit scores beside an F32 mask, included); element accesses that feed
 * the same arithmetic otherwise.
 */
#ifndef LLMQAT_FAKEQUANT_ATTN_H
#define LLMQAT_FAKEQUANT_ATTN_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward, one launch.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (unknown codes; float64; with a mask, a mask dtype that is neither the
 * scores' nor F32), FQ_ERR_SHAPE (rows or cols not positive; rows * cols overflows; B, H or T not positive; rows not a multiple of T;
 * rows != B * H * T; with a mask, a negative stride), FQ_ERR_NULL (scores, y), FQ_ERR_ARG (y on scores or the mask; stats on scores, the
 * mask or y), FQ_ERR_UNSUPPORTED (rows beyond one launch's grid). */
int fqs2_attn_softmax_fwd(const void* scores, const void* mask, void* y, float* stats, int64_t rows, int64_t cols, int64_t B, int64_t H,
                          int64_t T, int64_t mask_batch_stride, int64_t mask_row_stride, float inv, int scores_dtype, int mask_dtype,
                          void* stream);

/* Backward, one launch: dx [rows, cols] of ds from g, the forward's scores, mask, inv and stats.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE and FQ_ERR_SHAPE as the forward, FQ_ERR_NULL (g, scores, stats, dx),
 * FQ_ERR_ARG (dx on g, scores, the mask or stats), FQ_ERR_UNSUPPORTED (as the forward). */
int fqs2_attn_softmax_bwd(const void* g, const void* scores, const void* mask, const float* stats, void* dx, int64_t rows, int64_t cols,
                          int64_t B, int64_t H, int64_t T, int64_t mask_batch_stride, int64_t mask_row_stride, float inv, int scores_dtype,
                          int mask_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ATTN_H */
