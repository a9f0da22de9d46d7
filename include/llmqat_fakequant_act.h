/* llmqat_fakequant_act.h -- the activation entry points of libllmqat_fakequant.so (family prefix fqa_).
 *
 * The seven other headers' sets of entry points are recorded and stay as they are; the gated activation in the middle of a LLaMA MLP,
 * silu(gate) * up, whose result the down projection's activation quantizer reads, lives here, in the same library, under a prefix of its
 * own.  Conventions as in llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default stream), no allocation, no
 * synchronisation, 0 or a negative FQ_ERR_* code, the message of a refusal through the main header's last-error call.  The dtype codes
 * are the main header's.  No atomics and no workspace: two calls on the same inputs give the same bits.
 *
 * One dtype for all tensors: F32, BF16 or F16; float64 is refused.  gate, up and dy = dL/dy are [rows, cols] with unit-stride columns and a
 * row stride in elements of their own, at least cols (so the two halves of a [rows, 2 cols] tensor are served where they lie); y, dgate
 * and dup are contiguous [rows, cols].  All index arithmetic is 64-bit.  The arithmetic is fp32 with the roundings of the eager chain
 * F.silu(gate) * up and of its autograd; rb rounds to the dtype (nearest even) and back, the identity for F32:
 *
 *   sig = 1 / (1 + exp(-g))
 *   a   = g / (1 + exp(-g))                       ATen's silu: a division, not g * sig
 *   y   = rb( rb(a) * u )
 *   ds  = rb( dy * u )                            mul's backward, rounded as the chain stores it
 *   du  = rb( dy * rb(a) )                        the chain saves silu's ROUNDED output
 *   dg  = rb( ds * sig * (1 + g * (1 - sig)) )    ATen's silu_backward in its op order: (ds * sig) * fma(g, 1 - sig, 1), the one
 *                                                 contraction of ATen's device code
 *
 * Special values follow the chain and are not patched: silu(-inf) is NaN, silu(+inf) * 0 is NaN, a gate from which exp(-g) overflows
 * (every g <= -104) gives -0, a NaN stays in its element.  One departure, F16 only: where dg is a zero, ATen's kernel stores +0 for a
 * product of -0 in the remainder behind the last whole block of 4096 elements of its loop and -0 elsewhere; dg here keeps the product's sign.
 *
 * No alignment requirement: 16-byte loads and stores where every base pointer and every row pitch in bytes is 16-byte aligned and
 * cols * itemsize is a multiple of 16; element accesses that feed the same arithmetic otherwise.
 */
#ifndef LLMQAT_FAKEQUANT_ACT_H
#define LLMQAT_FAKEQUANT_ACT_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward, one launch: y = silu(gate) * up.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (unknown codes, float64), FQ_ERR_SHAPE (negative or zero rows / cols; a
 * stride below cols; rows * cols overflowing; (rows - 1) * stride + cols overflowing), FQ_ERR_NULL (gate, up, y), FQ_ERR_ARG (y is gate
 * or up), FQ_ERR_UNSUPPORTED (a shape one launch's grid does not hold). */
int fqa_swiglu_fwd(const void* gate, const void* up, void* y, int64_t rows, int64_t cols, int64_t gate_stride, int64_t up_stride, int dtype,
                   void* stream);

/* Backward, one launch: dgate and dup from dy, gate and up.  dgate NULL or dup NULL: that gradient is neither computed nor stored (dup
 * alone does not read up).  Not both may be NULL.
 *
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE, FQ_ERR_SHAPE (as the forward, dy_stride included), FQ_ERR_NULL (dy, gate,
 * up; dgate and dup both), FQ_ERR_ARG (dgate or dup is dy, gate or up; dgate is dup), FQ_ERR_UNSUPPORTED (a shape one launch's grid does
 * not hold). */
int fqa_swiglu_bwd(const void* dy, const void* gate, const void* up, void* dgate, void* dup, int64_t rows, int64_t cols, int64_t dy_stride,
                   int64_t gate_stride, int64_t up_stride, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_ACT_H */
