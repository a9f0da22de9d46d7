/* llmqat_fakequant_attn_decode.h -- the decode-attention entry points of libllmqat_fakequant.so (family prefix fqd_).
 *
 * The ten other headers' sets of entry points are recorded and stay as they are; the attention of a few new tokens over a long cache
 * (the reference's models/modeling_llama_quant.py:345-377 with past_key_value: the product q k^T, the division by sqrt(head_dim), the
 * additive mask, the clamp at finfo.min, the fp32 softmax, the product with v) lives here as one fused forward, in the same library,
 * under a prefix of its own.  Conventions as in llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default stream), no
 * allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message of a refusal through the main header's last-error call.
 * The dtype codes are the main header's.  No atomics: two calls on the same inputs give the same bits.  Forward only.
 *
 * Tensors.  q is [B, H, T, D], k and v are [B, H, S, D], one dtype ds: BF16 or F16; each is read where it lies through its element
 * strides for batch, head and token (not negative; last stride 1), so the views .view(b, t, nh, hd).transpose(1, 2) of a projection and
 * the contiguous result of a concatenation with a cache are served alike.  1 <= T <= 16; D is 64 or 128.  mask is NULL or [B, 1, T, S],
 * given as a base pointer, a batch stride and a row stride in elements (not negative; the batch stride may be 0), last stride 1; its
 * dtype dm is ds or F32 (mask_dtype is not looked at where mask is NULL).  out is [B, T, H, D] of ds, contiguous: the layout the output
 * projection consumes.  All index arithmetic is 64-bit.
 *
 * Arithmetic: llmqat_fakequant_attn.h's chain with the two products around it, in fp32 accumulation.  P = ds where dm is ds or the mask
 * is NULL, else F32; rb_X rounds to dtype X (nearest even) and back; MIN_P = the most negative finite value of P:
 *
 *   x   = rb_ds( sum_d q[t, d] k[s, d] )          the first product's own rounding
 *   a   = rb_P( rb_ds(x * inv) + m ),  z = a < MIN_P ? MIN_P : a          without a mask: z = rb_ds(x * inv), no clamp
 *   e_s = exp(z_s - max_s z)
 *   out[t, :] = rb_ds( (sum_s rb_ds(e_s) v[s, :]) / sum_s e_s )
 *
 * The maximum and the sum are kept online over tiles of keys, and S is cut into nsplit chunks whose partial results are merged in a
 * fixed order; the unnormalised e_s is rounded to ds as the second product's operand, where the reference rounds the normalised
 * probability.  The result is therefore held to an error bound against float64 beside the composed path's own,
 * not to its bits.  A NaN or +inf score makes its own query row NaN and no other.
 *
 * The work split is a function of B * H, S and cus, the device's compute-unit count (<= 0: 256, the MI355X's): give both calls the same.
 *
 * No alignment requirement: 16-byte loads where the bases of q, k, v and their strides in bytes are multiples of 16; 2-byte loads that
 * feed the same arithmetic otherwise.
 */
#ifndef LLMQAT_FAKEQUANT_ATTN_DECODE_H
#define LLMQAT_FAKEQUANT_ATTN_DECODE_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The workspace the forward needs, in bytes (0 where S is one chunk), and the number of chunks it will cut S into.
 *
 * Status, in this order: FQ_ERR_DTYPE (unknown code; a dtype that is not BF16 or F16), FQ_ERR_SHAPE (B, H or S not positive; T not in
 * 1 .. 16; D not 64 or 128; B * H * S overflows), FQ_ERR_NULL (bytes, nsplit). */
int fqd_attn_decode_workspace(int64_t B, int64_t H, int64_t T, int64_t D, int64_t S, int64_t cus, int dtype, size_t* bytes, int64_t* nsplit);

/* Forward: one launch, and a second small one where S is cut into more than one chunk.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (as above; with a mask, an unknown mask code or a mask dtype that is
 * neither ds nor F32), FQ_ERR_SHAPE (as above; a negative stride; a tensor's extent overflows), FQ_ERR_NULL (q, k, v, out), FQ_ERR_ARG
 * (out or the workspace at the base pointer of q, k, v or the mask, the workspace at out's: equal pointers are compared, as in the other
 * headers; buffers that overlap elsewhere are the caller's to avoid), FQ_ERR_UNSUPPORTED (a workspace that is NULL or smaller than
 * fqd_attn_decode_workspace's answer where that is not 0; B * H beyond one launch's grid). */
int fqd_attn_decode_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, void* workspace, size_t workspace_bytes,
                        int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_head_stride,
                        int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride,
                        int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H, int64_t T, int64_t S, int64_t D, int64_t cus,
                        float inv, int dtype, int mask_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ATTN_DECODE_H */
