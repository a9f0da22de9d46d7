/* llmqat_fakequant_attn_kvdecode.h -- the decode attention over a K/V cache of integer codes (family prefix fqk_).
 *
 * The other headers' sets of entry points are recorded and stay as they are.  llmqat_fakequant_attn_decode.h's operation, arithmetic,
 * work split and conventions (device pointers, a HIP stream, no allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the
 * message through the main header's last-error call, no atomics, forward only), with k and v given as what fq_sym_export writes for
 * the per-token K / V hooks: signed codes and one fp32 divisor t2 per token.  k and v never exist as 16-bit tensors.
 *
 * Tensors.  q is [B, H, T, D] of ds (BF16 or F16) by element strides, 1 <= T <= 16, D 64 or 128.  k_codes and v_codes are [B, H, S, D]
 * codes by BYTE strides for batch, head and token (not negative), a key's codes contiguous: code_bits 8 is int8, code_bits 4 is two's
 * complement nibbles, element 2 k in the low nibble of byte k (D / 2 bytes per key).  k_t2 and v_t2 are fp32 [B, S] by a batch stride
 * in elements, last stride 1.  mask, out and the workspace are the decode header's.
 *
 *   khat[s, d] = rb_ds( k_code[s, d] / k_t2[s] ),  vhat[s, d] = rb_ds( v_code[s, d] / v_t2[s] )
 *
 * with the correctly rounded fp32 quotient: the bits of the fake-quantized tensor the codes were exported from.
 *
 * Rotation.  cos and sin NULL: khat is the key.  Else they are tables [P, D] of ds, rows contiguous, and key s of batch b is rotated at
 * position p = key_positions[b * pos_batch_stride + s] (int64; pos_batch_stride 0: one row for every batch; key_positions NULL: p = s)
 * by llmqat_fakequant_rope.h's forward, partner d +- D / 2, with that header's rule for a position outside the table (p in [-P, 0)
 * wraps; any other p outside [0, P) makes the key NaN).  v is never rotated.  Behind the operands everything is the decode header's.
 *
 * No alignment requirement: wide loads where the bases of q, the codes and the tables and the byte strides of q and the codes are
 * multiples of 16; byte loads that feed the same arithmetic otherwise.  The work split is fqd_attn_decode_workspace's.
 */
#ifndef LLMQAT_FAKEQUANT_ATTN_KVDECODE_H
#define LLMQAT_FAKEQUANT_ATTN_KVDECODE_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The workspace the forward needs, in bytes (0 where S is one chunk), and the number of chunks it will cut S into.
 *
 * Status, in this order: FQ_ERR_DTYPE (unknown code; a dtype that is not BF16 or F16), FQ_ERR_BITS (code_bits not 8 or 4), FQ_ERR_SHAPE
 * (B, H or S not positive; T not in 1 .. 16; D not 64 or 128; B * H * S overflows), FQ_ERR_NULL (bytes, nsplit). */
int fqk_attn_kvdecode_workspace(int64_t B, int64_t H, int64_t T, int64_t D, int64_t S, int64_t cus, int dtype, int code_bits, size_t* bytes,
                                int64_t* nsplit);

/* Forward: one launch, and a second small one where S is cut into more than one chunk.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (as above; with a mask, an unknown mask code or a mask dtype that is
 * neither ds nor F32), FQ_ERR_BITS (as above), FQ_ERR_SHAPE (as above; a negative stride; with tables, P not positive; a tensor's
 * extent overflows), FQ_ERR_NULL (q, k_codes, k_t2, v_codes, v_t2, out; one table without the other; key_positions without tables),
 * FQ_ERR_ARG (out or the workspace at the base pointer of an input, the workspace at out's: equal pointers are compared),
 * FQ_ERR_UNSUPPORTED (a workspace that is NULL or smaller than fqk_attn_kvdecode_workspace's answer where that is not 0; B * H beyond
 * one launch's grid). */
int fqk_attn_kvdecode_fwd(const void* q, const void* k_codes, const float* k_t2, const void* v_codes, const float* v_t2, const void* mask,
                          const void* cos, const void* sin, const int64_t* key_positions, void* out, void* workspace, size_t workspace_bytes,
                          int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t k_batch_stride, int64_t k_head_stride,
                          int64_t k_token_stride, int64_t v_batch_stride, int64_t v_head_stride, int64_t v_token_stride, int64_t k_t2_batch_stride,
                          int64_t v_t2_batch_stride, int64_t mask_batch_stride, int64_t mask_row_stride, int64_t pos_batch_stride, int64_t P,
                          int64_t B, int64_t H, int64_t T, int64_t S, int64_t D, int64_t cus, float inv, int dtype, int mask_dtype, int code_bits,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ATTN_KVDECODE_H */
