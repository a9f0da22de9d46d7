// fq_loss_rows.h -- the row-softmax layer under the loss kernels (DESIGN.md sections 24 and 26): what fq_kd_loss.h (two logit tensors) and
// fq_ce_loss.h (one) share beyond the row layer of fq_rows.h, and what a further loss over rows of logits would stand on: the constants,
// the exponentials, the reference point and the size of the element path's group.  Launch shape, access paths and the entry points'
// common refusals are fq_rows.h's.  Retuning a constant here retunes every loss.
//
// Slots past the end of a row hold -inf: e^-inf = 0 adds nothing to a sum.
//
// Special values.  The reference point of a lane that has seen only -inf is 0 (loss_ref), so that -inf - max is never inf - inf; a
// row of only -inf ends in z = 0, and its loss is NaN as ATen's is.  v_max_f32 ignores a NaN operand, but e^(NaN - m) is NaN: the sum,
// hence the logsumexp, the row's loss and its gradient are NaN.  exp is v_exp_f32 on (x - m) * log2(e): the difference is taken first
// (exact or nearly so), so the argument's error is relative to the distance from the maximum, where the term's weight is small.
// Results below the fp32 normal range flush to zero.
#pragma once
#include "fq_rows.h"

namespace fq {

constexpr int LOSS_EG = 4;             // elements per group of the element path
constexpr float LOSS_LOG2E = 1.44269504088896340736f;
#define LOSS_NEG_INF (-__builtin_inff())

__device__ __forceinline__ float loss_exp(float d) { return __builtin_amdgcn_exp2f(d * LOSS_LOG2E); }
// e^d for the gradient, where an element's relative error counts whatever its size: d * log2(e) as an unevaluated sum hi + lo (lo: the
// product's rounding error and the fp32 constant's own, both proportional to |d|, which loss_exp leaves in the result as a relative error
// of about |d| 2^-24), v_exp_f32 on hi, lo applied to first order.  d = -inf: hi = -inf, lo = NaN, and the result is the 0 of 2^hi.
constexpr float LOSS_LOG2E_LO = 1.92596299e-8f;     // log2(e) - (float)log2(e)
constexpr float LOSS_LN2 = 0.693147180559945309417f;
__device__ __forceinline__ float loss_exp_acc(float d) {
    const float hi = d * LOSS_LOG2E;
    const float lo = __builtin_fmaf(d, LOSS_LOG2E_LO, __builtin_fmaf(d, LOSS_LOG2E, -hi));
    const float e = __builtin_amdgcn_exp2f(hi);
    return e == 0.0f ? 0.0f : __builtin_fmaf(e, lo * LOSS_LN2, e);
}
__device__ __forceinline__ float loss_ref(float m) { return m == LOSS_NEG_INF ? 0.0f : m; }

}  // namespace fq
