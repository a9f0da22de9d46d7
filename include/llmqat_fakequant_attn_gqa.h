/* llmqat_fakequant_attn_gqa.h -- grouped-query attention (family prefix fqh_): the decode, codes-cache and prefill attention with
 * fewer K/V heads than query heads.
 *
 * The other headers' sets of entry points are recorded and stay as they are.  Each function here is the function of the same name in
 * llmqat_fakequant_attn_decode.h (fqd_), llmqat_fakequant_attn_kvdecode.h (fqk_) or llmqat_fakequant_attn_prefill.h (fqp_) with one
 * more argument, Hkv, behind H: q and out keep their H heads, k and v (or their codes) are [B, Hkv, S, D] with the head stride over
 * those Hkv heads, H % Hkv == 0, and query head h attends to K/V head h / (H / Hkv): what the ungrouped function computes on k and v
 * with every head repeated H / Hkv times in place.  Operation, arithmetic, tensors, strides, mask, conventions (device pointers, a HIP
 * stream, no allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message through the main header's last-error call, no
 * atomics, forward only) are those headers'.
 *
 * Decode work split.  With G = H / Hkv, HP = min(G, 16 / T) query heads of one K/V head share a workgroup and NP = ceil(G / HP) such
 * packs serve a K/V head: K and V (codes: their dequantisation and rotation too) are read once per pack.  The split along S is
 * fqd_attn_decode_workspace's rule asked with B * Hkv * NP workgroups, the workspace fp32 [B * Hkv * NP, nsplit, HP * T, D + 2].  Per
 * query row the arithmetic is the ungrouped function's; where both cut S into one chunk the results are equal to the bit.
 */
#ifndef LLMQAT_FAKEQUANT_ATTN_GQA_H
#define LLMQAT_FAKEQUANT_ATTN_GQA_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The workspace the decode forward needs, in bytes (0 where S is one chunk), and the number of chunks it will cut S into.
 *
 * Status, in this order: FQ_ERR_DTYPE (unknown code; a dtype that is not BF16 or F16), FQ_ERR_SHAPE (B, H or S not positive; Hkv not
 * positive or not a divisor of H; T not in 1 .. 16; D not 64 or 128; B * H * S overflows), FQ_ERR_NULL (bytes, nsplit). */
int fqh_attn_decode_workspace(int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t D, int64_t S, int64_t cus, int dtype, size_t* bytes,
                              int64_t* nsplit);

/* fqd_attn_decode_fwd over k, v of Hkv heads.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (as above; with a mask, an unknown mask code or a mask dtype that is
 * neither ds nor F32), FQ_ERR_SHAPE (as above; a negative stride; a tensor's extent overflows), FQ_ERR_NULL (q, k, v, out), FQ_ERR_ARG
 * (out or the workspace at the base pointer of an input, the workspace at out's), FQ_ERR_UNSUPPORTED (a workspace that is NULL or
 * smaller than fqh_attn_decode_workspace's answer where that is not 0; B * Hkv * NP beyond one launch's grid). */
int fqh_attn_decode_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, void* workspace, size_t workspace_bytes,
                        int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_head_stride,
                        int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, int64_t mask_batch_stride,
                        int64_t mask_row_stride, int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t S, int64_t D, int64_t cus, float inv,
                        int dtype, int mask_dtype, void* stream);

/* fqk_attn_kvdecode_workspace for codes of Hkv heads: fqh_attn_decode_workspace's statuses with FQ_ERR_BITS (code_bits not 8 or 4)
 * between FQ_ERR_DTYPE and FQ_ERR_SHAPE. */
int fqh_attn_kvdecode_workspace(int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t D, int64_t S, int64_t cus, int dtype, int code_bits,
                                size_t* bytes, int64_t* nsplit);

/* fqk_attn_kvdecode_fwd over codes of Hkv heads (k_t2, v_t2, the tables and the positions are per token and stay as they are).
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE, FQ_ERR_BITS, FQ_ERR_SHAPE (fqh_attn_decode_workspace's; a negative
 * stride; with tables, P not positive; a tensor's extent overflows), FQ_ERR_NULL (q, k_codes, k_t2, v_codes, v_t2, out; one table
 * without the other; key_positions without tables), FQ_ERR_ARG (as above), FQ_ERR_UNSUPPORTED (the workspace against
 * fqh_attn_kvdecode_workspace's answer; B * Hkv * NP beyond one launch's grid). */
int fqh_attn_kvdecode_fwd(const void* q, const void* k_codes, const float* k_t2, const void* v_codes, const float* v_t2, const void* mask,
                          const void* cos, const void* sin, const int64_t* key_positions, void* out, void* workspace, size_t workspace_bytes,
                          int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_head_stride,
                          int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, int64_t k_t2_batch_stride,
                          int64_t v_t2_batch_stride, int64_t mask_batch_stride, int64_t mask_row_stride, int64_t pos_batch_stride, int64_t P,
                          int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t S, int64_t D, int64_t cus, float inv, int dtype, int mask_dtype,
                          int code_bits, void* stream);

/* fqp_attn_prefill_fwd over k, v of Hkv heads: the same launch, K and V read from head h / (H / Hkv).  Equal to the ungrouped function
 * on the repeated k, v to the bit at every shape.
 *
 * Status, in this order and before any HIP call: fqp_attn_prefill_fwd's, with FQ_ERR_SHAPE for an Hkv that is not positive or does
 * not divide H behind the check that B, H, T, S are positive. */
int fqh_attn_prefill_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, int64_t q_batch_stride, int64_t q_head_stride,
                         int64_t q_token_stride, int64_t k_batch_stride, int64_t k_head_stride, int64_t k_token_stride, int64_t v_batch_stride,
                         int64_t v_head_stride, int64_t v_token_stride, int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H,
                         int64_t Hkv, int64_t T, int64_t S, int64_t D, float inv, int dtype, int mask_dtype, int causal, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ATTN_GQA_H */
