/* llmqat_fakequant_attn_cached_codes.h -- the decode attention over an in-place K/V cache of integer codes with device lengths (family
 * prefix fqw_).
 *
 * The other headers' sets of entry points are recorded and stay as they are.  llmqat_fakequant_attn_cached.h's call on
 * llmqat_fakequant_attn_kvdecode.h's operands: the caches hold what fq_sym_export writes for the per-token K / V hooks, codes
 * k_code_cache, v_code_cache [B, Hkv, Smax, D] (code_bits 8: int8) or [B, Hkv, Smax, D / 2] (code_bits 4: element 2 k in the low nibble
 * of byte k) beside one fp32 divisor per token, k_t2_cache, v_t2_cache [B, Smax].  All four are preallocated by the caller;
 * cache_lens [B] (int32, on the device) says how many keys of each batch row are valid.  One call brings T <= 16 new tokens, q
 * [B, H, T, D], their codes [B, Hkv, T, D or D / 2] and divisors [B, T], and for batch row b with len = cache_lens[b]
 *
 *   1. writes the new code rows and divisors into rows len .. len + T - 1 of the four caches, bit for bit, and
 *   2. lets query row t attend to the keys start_b <= s <= len + t of the updated cache (start_b = cache_starts[b], 0 where
 *      cache_starts is NULL: left padding), causal among the new tokens,
 *
 * in ONE launch (a second small one where the keys are cut into chunks).  The operands are khat = rope(rb(code / t2)) with the tables'
 * row s - start_b (cos NULL: no rotation) and vhat = rb(code / t2), made in registers with llmqat_fakequant_attn_kvdecode.h's
 * arithmetic; there is no positions tensor.  Everything behind the operands is llmqat_fakequant_attn_cached.h's: no mask, x and x * inv
 * rounded to ds, no clamp, an unseen key -inf in front of the online fp32 softmax.  The lengths are read on the device and never on the
 * host; the call does not advance them.  H % Hkv == 0; query head h reads K/V head h / (H / Hkv), packed as llmqat_fakequant_attn_gqa.h
 * says.  Conventions (device pointers, a HIP stream, no allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message
 * through the main header's last-error call, no atomics, forward only, 64-bit index arithmetic) are the other headers'.
 *
 * Tensors.  q is ds, BF16 or F16, read through its element strides for batch, head and token (last stride 1).  The new codes and the
 * code caches are read (the caches also written) where they lie through their BYTE strides for batch, head and token (not negative;
 * bytes of a row contiguous).  The divisors have a batch stride in elements and contiguous rows.  cos, sin: [P, D] of ds, contiguous,
 * both or neither; P >= Smax is the caller's to check (a position at or past P rotates with NaN, the rotary header's rule).  out is
 * [B, T, H, D], contiguous.
 *
 * The contract is 0 <= start_b <= len_b and len_b + T <= Smax.  The kernel clamps on its own: a negative length counts as 0, one above
 * Smax as Smax, a start is brought into [0, len_b]; a new row that would land at or past Smax is not stored and still takes part in this
 * call's attention.  No address outside the tensors is formed, whatever the int32s hold.
 *
 * The launch shape is static: the grid, nsplit and the workspace are functions of B, H, Hkv, T, Smax and cus (the device's compute-unit
 * count; <= 0: 256) alone: fqu_attn_cached_workspace's.
 *
 * No alignment requirement: 16-byte loads and stores where the bases of q, the code tensors and the tables and their strides in bytes
 * are multiples of 16; byte ones (2-byte for q and the tables) that move the same values otherwise.
 */
#ifndef LLMQAT_FAKEQUANT_ATTN_CACHED_CODES_H
#define LLMQAT_FAKEQUANT_ATTN_CACHED_CODES_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The workspace the forward needs, in bytes (0 where nsplit is 1), and the number of chunks.
 *
 * Status, in this order: FQ_ERR_DTYPE (unknown code; a dtype that is not BF16 or F16), FQ_ERR_BITS (code_bits not 8 or 4), FQ_ERR_SHAPE
 * (B, H or Smax not positive; Hkv not positive or not a divisor of H; T not in 1 .. 16; D not 64 or 128; Smax + T beyond 2^31 - 1;
 * B * H * Smax overflows), FQ_ERR_NULL (bytes, nsplit). */
int fqw_attn_cached_codes_workspace(int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t D, int64_t Smax, int64_t cus, int dtype, int code_bits,
                                    size_t* bytes, int64_t* nsplit);

/* Forward: appends and attends.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE, FQ_ERR_BITS, FQ_ERR_SHAPE (as above; a negative stride; P not positive
 * beside tables; a tensor's extent overflows), FQ_ERR_NULL (q, the four new tensors, the four caches, cache_lens, out; cos without sin
 * or sin without cos; cache_starts may be NULL), FQ_ERR_ARG (the byte range of q or of a new tensor overlaps that of a cache: the append
 * would race the reads; two caches overlap; out or the workspace at the base pointer of another argument), FQ_ERR_UNSUPPORTED (a
 * workspace that is NULL or smaller than fqw_attn_cached_codes_workspace's answer where that is not 0; B * Hkv * NP beyond one launch's
 * grid). */
int fqw_attn_cached_codes_fwd(const void* q, const void* k_codes_new, const float* k_t2_new, const void* v_codes_new, const float* v_t2_new,
                              void* k_code_cache, float* k_t2_cache, void* v_code_cache, float* v_t2_cache, const int32_t* cache_lens,
                              const int32_t* cache_starts, const void* cos, const void* sin, void* out, void* workspace, size_t workspace_bytes,
                              int64_t q_batch_stride, int64_t q_head_stride, int64_t q_token_stride, int64_t kn_batch_stride,
                              int64_t kn_head_stride, int64_t kn_token_stride, int64_t vn_batch_stride, int64_t vn_head_stride,
                              int64_t vn_token_stride, int64_t kc_batch_stride, int64_t kc_head_stride, int64_t kc_token_stride,
                              int64_t vc_batch_stride, int64_t vc_head_stride, int64_t vc_token_stride, int64_t k_t2_new_batch_stride,
                              int64_t v_t2_new_batch_stride, int64_t k_t2_cache_batch_stride, int64_t v_t2_cache_batch_stride, int64_t P, int64_t B,
                              int64_t H, int64_t Hkv, int64_t T, int64_t Smax, int64_t D, int64_t cus, float inv, int dtype, int code_bits,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ATTN_CACHED_CODES_H */
