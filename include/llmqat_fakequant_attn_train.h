/* llmqat_fakequant_attn_train.h -- the training-attention entry points of libllmqat_fakequant.so (family prefix fqg_).
 *
 * The twelve other headers' sets of entry points are recorded and stay as they are; the attention call that needs a gradient (the
 * student's, in every layer of every step) lives here as a fused forward that also writes two floats per query row, and a fused
 * backward of two launches, in the same library, under a prefix of its own.  No [B, H, T, S] tensor exists in either direction.
 * Conventions as in llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default stream), no allocation, no synchronisation, 0
 * or a negative FQ_ERR_* code, the message of a refusal through the main header's last-error call.  The dtype codes are the main
 * header's.  No atomics: two calls on the same inputs give the same bits.
 *
 * Tensors: llmqat_fakequant_attn_prefill.h's.  q is [B, H, T, D], k and v are [B, H, S, D], one dtype ds: BF16 or F16, each read
 * through its element strides for batch, head and token (not negative; last stride 1); D is 64 or 128, T >= 1, S >= 1.  mask is NULL
 * or [B, 1, T, S] by a batch stride and a row stride in elements, in ds or F32.  out is [B, T, H, D] of ds, contiguous.  stats is
 * F32 [B, H, T, 2], contiguous: the row's maximum of z and the fp32 sum of the unrounded exponentials exp(z - max), the pair of
 * llmqat_fakequant_attn.h.  All index arithmetic is 64-bit.
 *
 * Arithmetic of the forward: llmqat_fakequant_attn_prefill.h's, to the bit.  Of the backward: x, a, z are recomputed as the forward
 * computed them, p = exp(z - max) (1 / sum) from stats; g = dout . v, delta = sum_s p g (summed over the keys in a walk of its own; out is not read), d = (g - delta) p, times the gradient of
 * the clamp under a mask (1 where a > finfo.min, 1/2 where equal, 0 below), times inv, all in fp32 and unrounded.  Two roundings to
 * ds stand in the backward, each in front of a matrix product: rb(p) in dv = sum_t rb(p) dout, and ds = rb(d inv) in dq = sum_s ds k,
 * dk = sum_t ds q.  The sums are fp32; each output is rounded once.  Keys excluded by causal have p = 0 exactly.  The results are held to
 * error bounds against float64 beside the composed path's own, not to its bits.
 */
#ifndef LLMQAT_FAKEQUANT_ATTN_TRAIN_H
#define LLMQAT_FAKEQUANT_ATTN_TRAIN_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward: one launch.  fqp_attn_prefill_fwd's arguments and result, plus stats (NULL: not written).
 *
 * Status, in this order and before any HIP call: fqp_attn_prefill_fwd's, with stats among the pointers out is compared with and
 * stats compared with the inputs (FQ_ERR_ARG). */
int fqg_attn_train_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, float* stats, int64_t q_batch_stride,
                       int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride,
                       int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, int64_t mask_batch_stride,
                       int64_t mask_row_stride, int64_t B, int64_t H, int64_t T, int64_t S, int64_t D, float inv, int dtype, int mask_dtype,
                       int causal, void* stream);

/* Backward: two launches on `stream`, the second (dk, dv) behind the first (dq, delta).  out and dout are [B, H, T, D] of ds by
 * element strides like q (the forward's out is such a view of its [B, T, H, D] memory).  delta is a caller-allocated F32 workspace of
 * B * H * T elements.  dq is [B, T, H, D], dk and dv are [B, S, H, D], of ds, contiguous; every element is written exactly once.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE and FQ_ERR_SHAPE as the forward's (the strides of out and dout
 * included), FQ_ERR_NULL (q, k, v, out, dout, stats, delta, dq, dk, dv), FQ_ERR_ARG (an output or delta at the base pointer of an
 * input or of another output; causal together with a mask), FQ_ERR_UNSUPPORTED (B * H, the query tiles or the key tiles beyond one
 * launch's grid). */
int fqg_attn_train_bwd(const void* q, const void* k, const void* v, const void* mask, const void* out, const void* dout, const float* stats,
                       float* delta, void* dq, void* dk, void* dv, int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride,
                       int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride,
                       int64_t v_token_stride, int64_t out_batch_stride, int64_t out_head_stride, int64_t out_token_stride,
                       int64_t dout_batch_stride, int64_t dout_head_stride, int64_t dout_token_stride, int64_t mask_batch_stride,
                       int64_t mask_row_stride, int64_t B, int64_t H, int64_t T, int64_t S, int64_t D, float inv, int dtype, int mask_dtype,
                       int causal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ATTN_TRAIN_H */
