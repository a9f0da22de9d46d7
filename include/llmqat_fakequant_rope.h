/* llmqat_fakequant_rope.h -- the rotary position embedding entry points of libllmqat_fakequant.so (family prefix fqr_).
 *
 * The eight other headers' sets of entry points are recorded and stay as they are; the rotary embedding that every decoder layer applies
 * to q and k between the projections and the attention product (the reference's apply_rotary_pos_emb) lives here, in the same library,
 * under a prefix of its own.  Conventions as in llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default stream), no
 * allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message of a refusal through the main header's last-error call.
 * The dtype codes are the main header's.  No atomics and no workspace: two calls on the same inputs give the same bits.
 *
 * Tensors.  q is [B, Hq, T, D] and k is [B, Hk, T, D] (Hq and Hk may differ), D even, in one dtype: F32, BF16 or F16; float64 is refused.
 * The last stride is 1; the three other strides, in elements and not negative, are given per tensor as (batch, head, token), so a
 * transposed view over [B, T, H * D] memory and a part of a fused qkv projection are read where they lie.  The outputs are dense, in their
 * input's dimension order: the dimensions of size 1 keep their place in (batch, head, token), the others are ordered by the input's
 * stride, a larger stride outside (equal or zero strides keep their order); fqr_rope_dense_strides gives these strides.  This is the
 * layout the eager chain returns.  All index arithmetic is 64-bit.
 *
 * Tables.  cos and sin are [P, D] with contiguous rows, either in the tensors' dtype or in F32; an F32 table is rounded to the dtype
 * in the kernel, as the reference's .to(dtype=x.dtype) does.  Both halves of a row are used as given.
 *
 * Positions.  int64 [B, T] (pos_batch_stride = T), [1, T] for every batch (pos_batch_stride = 0), or NULL: the token's index.  A
 * position p in [-P, 0) means p + P; one outside [-P, P) is never followed outside the table (row 0 is read in its place), and every
 * output of that token, in every head of q and k, is NaN.
 *
 * Arithmetic: fp32 with the eager chain's roundings; rb rounds to the dtype (nearest even) and back, the identity for F32.  h = D / 2,
 * c and s the table rows of the token's position (rounded to the dtype), x one head of q or k, g one head of an incoming gradient:
 *
 *   y[j]      = rb( rb(x[j]     * c[j]    ) + rb( (-x[j + h]) * s[j]     ) )        j < h
 *   y[j + h]  = rb( rb(x[j + h] * c[j + h]) + rb(   x[j]      * s[j + h] ) )
 *   a = rb(g * c), b = rb(g * s)                    elementwise over the head
 *   dx[j]     = rb( a[j]     + b[j + h] ) + (+0)
 *   dx[j + h] = rb( a[j + h] + (-b[j])  ) + (+0)   autograd adds the zero-padded gradients of the two slices: a zero gradient is +0
 *
 * Special values follow the chain and are not patched.
 *
 * q and k in two dtypes.  Under autocast the reference's k comes out of its fp32 quantizer while q is 16-bit, and the tables are cast to
 * v's dtype, fp32: the chain then promotes.  That case is served as the chain computes it: one of q_dtype and k_dtype is F32, the other
 * BF16 or F16, the tables are F32 and are used as they are.  Both results are F32 (rb above is the identity; the 16-bit values enter
 * exactly).  Backward, both incoming gradients are F32, dq and dk have their tensor's dtype, and for the 16-bit side rb above rounds to
 * that dtype: autograd rounds g * c and g * s to it and sums the slices in it.
 *
 * No alignment requirement: 16-byte loads and stores where every base pointer (tensors and tables) and every stride in bytes is 16-byte
 * aligned and h * itemsize is a multiple of 16; element accesses that feed the same arithmetic otherwise.
 */
#ifndef LLMQAT_FAKEQUANT_ROPE_H
#define LLMQAT_FAKEQUANT_ROPE_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The strides (batch, head, token) of the dense output that belongs to an input of shape [B, H, T, D] with the given strides -> out[3].
 * Host arithmetic only.  FQ_ERR_SHAPE for non-positive dims, FQ_ERR_NULL for out. */
int fqr_rope_dense_strides(int64_t B, int64_t H, int64_t T, int64_t D, int64_t stride_b, int64_t stride_h, int64_t stride_t, int64_t* out);

/* Forward, one launch for q and k.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (unknown codes; float64; two 16-bit dtypes that differ; tables that are not F32
 * beside two dtypes; a table dtype that is neither the tensors' nor F32),
 * FQ_ERR_SHAPE (B, Hq, Hk, T or D not positive; odd D; P <= 0; a negative stride; pos_batch_stride neither 0 nor T; an element count, an
 * extent or P * D that overflows), FQ_ERR_NULL (q, k, q_out, k_out, cos, sin), FQ_ERR_ARG (an output that is an input, a table or the
 * other output), FQ_ERR_UNSUPPORTED (B * T beyond one launch's grid; (Hq + Hk) * D / 2 beyond 2^30). */
int fqr_rope_fwd(const void* q, const void* k, void* q_out, void* k_out, const void* cos, const void* sin, const int64_t* positions,
                 int64_t pos_batch_stride, int64_t B, int64_t Hq, int64_t Hk, int64_t T, int64_t D, int64_t P, int64_t q_stride_b,
                 int64_t q_stride_h, int64_t q_stride_t, int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t, int q_dtype,
                 int k_dtype, int table_dtype, void* stream);

/* Backward, one launch: dq and dk from the gradients dq_out and dk_out of the forward's outputs, the tables and the positions; neither q
 * nor k is needed.  dq NULL or dk NULL: that side is neither read, computed nor stored (its incoming gradient may be NULL too).  Not both.
 * g*_stride_*: the strides of the incoming gradients (last stride 1); q_stride_* / k_stride_*: the strides of the forward's q and k,
 * which give the dimension order of the dense dq and dk.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE, FQ_ERR_SHAPE (as the forward, the gradients' strides included),
 * FQ_ERR_NULL (cos, sin; dq and dk both; dq_out where dq is asked for, dk_out where dk is), FQ_ERR_ARG (dq or dk is a gradient read by
 * this launch or a table; dq is dk), FQ_ERR_UNSUPPORTED (as the forward). */
int fqr_rope_bwd(const void* dq_out, const void* dk_out, void* dq, void* dk, const void* cos, const void* sin, const int64_t* positions,
                 int64_t pos_batch_stride, int64_t B, int64_t Hq, int64_t Hk, int64_t T, int64_t D, int64_t P, int64_t gq_stride_b,
                 int64_t gq_stride_h, int64_t gq_stride_t, int64_t gk_stride_b, int64_t gk_stride_h, int64_t gk_stride_t,
                 int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_t, int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                 int q_dtype, int k_dtype, int table_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ROPE_H */
