/* llmqat_fakequant_attn_prefill.h -- the prefill-attention entry point of libllmqat_fakequant.so (family prefix fqp_).
 *
 * The eleven other headers' sets of entry points are recorded and stay as they are; the attention of a whole sequence, or of a long
 * chunk of new tokens over a cache (the reference's models/modeling_llama_quant.py:345-377: the product q k^T, the division by
 * sqrt(head_dim), the additive mask, the clamp at finfo.min, the fp32 softmax, the product with v), lives here as one fused forward, in
 * the same library, under a prefix of its own.  Conventions as in llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default
 * stream), no allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message of a refusal through the main header's
 * last-error call.  The dtype codes are the main header's.  No atomics, no workspace: two calls on the same inputs give the same bits.
 * Forward only.
 *
 * Tensors.  q is [B, H, T, D], k and v are [B, H, S, D], one dtype ds: BF16 or F16; each is read where it lies through its element
 * strides for batch, head and token (not negative; last stride 1).  T >= 1 (llmqat_fakequant_attn_decode.h is the faster one for
 * T <= 16 over a long cache: it splits S); D is 64 or 128.  mask is NULL or [B, 1, T, S], given as a base pointer, a batch stride and a
 * row stride in elements (not negative; the batch stride may be 0), last stride 1; its dtype dm is ds or F32 (mask_dtype is not looked
 * at where mask is NULL).  out is [B, T, H, D] of ds, contiguous: the layout the output projection consumes.  All index arithmetic is
 * 64-bit.
 *
 * Arithmetic: llmqat_fakequant_attn_decode.h's, to the letter (x, a, z, e_s, one division, one output rounding), with the maximum and
 * the sum kept online over tiles of 32 keys in key order.  The result is held to an error bound against float64 beside the composed
 * path's own, not to its bits.  A NaN or +inf score makes its own query row NaN and no other.
 *
 * causal != 0 (mask must be NULL, T <= S): query row t attends to the keys s <= S - T + t and to no others, as under the additive
 * causal mask with a past of S - T keys; the excluded keys have weight exactly 0 and are not read where a whole tile of them lies
 * past a workgroup's last row, the visible ones go through the chain without a mask (no clamp).
 *
 * No alignment requirement: 16-byte loads where the bases of q, k, v and their strides in bytes are multiples of 16, 2-byte loads that
 * feed the same arithmetic otherwise; the mask likewise (16 bytes of F32, 8 bytes of ds).
 */
#ifndef LLMQAT_FAKEQUANT_ATTN_PREFILL_H
#define LLMQAT_FAKEQUANT_ATTN_PREFILL_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward: one launch.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (an unknown code; a dtype that is not BF16 or F16; with a mask, an
 * unknown mask code or a mask dtype that is neither ds nor F32), FQ_ERR_SHAPE (B, H, T or S not positive; D not 64 or 128; a negative
 * stride; B * H * T or a tensor's extent overflows; causal with T > S), FQ_ERR_NULL (q, k, v, out), FQ_ERR_ARG (out at the base
 * pointer of q, k, v or the mask: equal pointers are compared, as in the other headers; causal together with a mask),
 * FQ_ERR_UNSUPPORTED (B * H or the number of query tiles beyond one launch's grid). */
int fqp_attn_prefill_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, int64_t q_batch_stride,
                         int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_head_stride,
                         int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride,
                         int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H, int64_t T, int64_t S, int64_t D,
                         float inv, int dtype, int mask_dtype, int causal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ATTN_PREFILL_H */
