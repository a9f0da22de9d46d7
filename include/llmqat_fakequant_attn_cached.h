/* llmqat_fakequant_attn_cached.h -- the decode attention over an in-place K/V cache with device lengths (family prefix fqu_).
 *
 * The other headers' sets of entry points are recorded and stay as they are.  The caches k_cache, v_cache [B, Hkv, Smax, D] are
 * preallocated by the caller; cache_lens [B] (int32, on the device) says how many keys of each batch row are valid.  One call brings
 * T <= 16 new tokens, q [B, H, T, D] and k_new, v_new [B, Hkv, T, D] (k already rotated), and for batch row b with len = cache_lens[b]
 *
 *   1. writes k_new[b], v_new[b] into rows len .. len + T - 1 of the caches, bit for bit, and
 *   2. lets query row t attend to the keys start_b <= s <= len + t of the updated cache (start_b = cache_starts[b], 0 where
 *      cache_starts is NULL: left padding), causal among the new tokens,
 *
 * in ONE launch (a second small one where the keys are cut into chunks).  The lengths are read on the device and never on the host; the
 * call does not advance them.  Arithmetic: llmqat_fakequant_attn_decode.h's without a mask (x and x * inv rounded to ds, no clamp), an
 * unseen key being -inf in front of the softmax: what fqh_attn_prefill_fwd computes with causal = 1 on the concatenation of the len
 * valid rows and the new ones.  H % Hkv == 0; query head h reads K/V head h / (H / Hkv), packed as llmqat_fakequant_attn_gqa.h says.
 * Conventions (device pointers, a HIP stream, no allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message through the
 * main header's last-error call, no atomics, forward only, 64-bit index arithmetic) are the other headers'.
 *
 * Tensors.  One dtype ds, BF16 or F16.  q, k_new, v_new, k_cache, v_cache are read (the caches also written) where they lie through
 * their element strides for batch, head and token (not negative; last stride 1).  out is [B, T, H, D], contiguous.
 *
 * The contract is 0 <= start_b <= len_b and len_b + T <= Smax.  The host cannot see the lengths, so the kernel clamps on its own: a
 * negative length counts as 0, one above Smax as Smax, a start is brought into [0, len_b]; a new row that would land at or past Smax is
 * not stored and still takes part in this call's attention.  No address outside the tensors is formed, whatever the int32s hold.
 *
 * The launch shape is static: the grid, nsplit and the workspace are functions of B, H, Hkv, T, Smax and cus (the device's compute-unit
 * count; <= 0: 256) alone; inside the kernel every batch row's own len_b + T keys are cut into up to nsplit chunks.
 *
 * No alignment requirement: 16-byte loads and stores where the bases of q, k_new, v_new, k_cache, v_cache and their strides in bytes
 * are multiples of 16; 2-byte ones that move the same values otherwise.
 */
#ifndef LLMQAT_FAKEQUANT_ATTN_CACHED_H
#define LLMQAT_FAKEQUANT_ATTN_CACHED_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The workspace the forward needs, in bytes (0 where nsplit is 1), and the number of chunks: fqh_attn_decode_workspace's answer for
 * S = Smax.
 *
 * Status, in this order: FQ_ERR_DTYPE (unknown code; a dtype that is not BF16 or F16), FQ_ERR_SHAPE (B, H or Smax not positive; Hkv not
 * positive or not a divisor of H; T not in 1 .. 16; D not 64 or 128; Smax + T beyond 2^31 - 1, the int32 lengths' range; B * H * Smax
 * overflows), FQ_ERR_NULL (bytes, nsplit). */
int fqu_attn_cached_workspace(int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t D, int64_t Smax, int64_t cus, int dtype, size_t* bytes,
                              int64_t* nsplit);

/* Forward: appends and attends.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE, FQ_ERR_SHAPE (as above; a negative stride; a tensor's extent overflows),
 * FQ_ERR_NULL (q, k_new, v_new, k_cache, v_cache, cache_lens, out; cache_starts may be NULL), FQ_ERR_ARG (the byte range of q, k_new or
 * v_new, by its strides, overlaps that of a cache: the append would race the reads; k_cache at v_cache; out or the workspace at the
 * base pointer of another argument), FQ_ERR_UNSUPPORTED (a workspace that is NULL or smaller than fqu_attn_cached_workspace's answer
 * where that is not 0; B * Hkv * NP beyond one launch's grid). */
int fqu_attn_cached_fwd(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int32_t* cache_lens,
                        const int32_t* cache_starts, void* out, void* workspace, size_t workspace_bytes, int64_t q_batch_stride,
                        int64_t q_head_stride, int64_t q_token_stride, int64_t kn_batch_stride, int64_t kn_head_stride, int64_t kn_token_stride,
                        int64_t vn_batch_stride, int64_t vn_head_stride, int64_t vn_token_stride, int64_t kc_batch_stride, int64_t kc_head_stride,
                        int64_t kc_token_stride, int64_t vc_batch_stride, int64_t vc_head_stride, int64_t vc_token_stride, int64_t B, int64_t H,
                        int64_t Hkv, int64_t T, int64_t Smax, int64_t D, int64_t cus, float inv, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ATTN_CACHED_H */
