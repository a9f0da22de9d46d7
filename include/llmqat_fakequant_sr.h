/* llmqat_fakequant_sr.h -- MX fake quantization with stochastic rounding: the entry points of libllmqat_fakequant.so for the tensor whose
 * rounding error must average out, the gradient (family prefix fqs_).
 *
 * The main header's set of entry points and the training header's are recorded and stay as they are; these live in the same library
 * under a prefix of their own.  Conventions as in llmqat_fakequant.h: device pointers, a HIP stream (NULL: the default stream), no
 * allocation, no synchronisation, 0 or a negative FQ_ERR_* code, the message of a refusal through the main header's last-error call.  The
 * dtype, format and flag codes are the main header's.
 *
 * Semantics.  Per block of 32 elements everything up to the shared exponent is the nearest forward's: the amax from the bit patterns, a
 * NaN / Inf in the block makes its 32 outputs NaN, E by the floor rule or (FQ_MX_FLAG_CEIL) the ceil rule, t = v * 2^-E, the binade of
 * |t| clamped at the format's smallest normal one.  Only the rounding of a = |t| / quantum (exact in fp32) differs:
 *     n = floor(a), f = a - n, up = float(R16) < f * 65536, r = n + up           (R16 in [0, 65535]: the element's random number)
 * r then takes the nearest forward's path: a carry into the next binade lands on the grid, saturation at max-normal, the input's sign,
 * one rounding to the dtype.  So a value on the grid is unchanged for every seed, every output is one of the two grid neighbours of |t|,
 * and P(up) = ceil(f * 2^16) / 2^16 -- exactly unbiased where f has at most 16 fractional bits (every bf16 / fp16 element within 2^9 of
 * its block's amax), a bias below 2^-16 quantum otherwise.  Under FQ_MX_FLAG_CEIL no element of a finite block saturates and E[y] = v
 * holds for the whole block; under the floor rule the top binade still clips, as in the nearest forward.
 *
 * The random numbers are Philox4x32-10 and depend only on (seed, stream_id, i), i the element's flat row-major index in the contiguous
 * [rows, cols] tensor (i = r * cols + c for both axes):
 *     key = (seed & 0xFFFFFFFF, seed >> 32), counter = (c & 0xFFFFFFFF, c >> 32, stream_id & 0xFFFFFFFF, stream_id >> 32), c = i >> 3
 *     j = i & 7: R16 = (word[j >> 1] >> 16 * (j & 1)) & 0xFFFF
 * Multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; per round hi0:lo0 = M0 * c0, hi1:lo1 = M1 * c2,
 * c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), then the key is bumped.  Any seed and stream_id are valid.  A launch captured into a
 * hipGraph carries its seed and stream_id: a replay repeats its noise.
 */
#ifndef LLMQAT_FAKEQUANT_SR_H
#define LLMQAT_FAKEQUANT_SR_H

#include "llmqat_fakequant.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The row axis: blocks of 32 consecutive elements of the last dimension; x, y contiguous [rows, cols].
 *   fmt     any of the five FQ_MX_* formats;  dtype  FQ_DTYPE_BF16 / F16 / F32;  flags  0 or FQ_MX_FLAG_CEIL, any other bit: FQ_ERR_ARG
 * Status, in this order and before any HIP call: FQ_ERR_DTYPE (float64, unknown codes), FQ_ERR_ARG (unknown fmt, flag bits),
 * FQ_ERR_SHAPE (negative shape, cols not a multiple of 32, overflowing shape), 0 without a launch for an empty shape, FQ_ERR_NULL,
 * FQ_ERR_ARG (y == x), FQ_ERR_UNSUPPORTED (x / y not 16-byte aligned, more vectors than one launch's grid holds). */
int fqs_mx_fwd(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, int flags, uint64_t seed, uint64_t stream_id, void* stream);

/* The column axis: the block is the 32 elements (32k .. 32k + 31, c) of one column, as in the training header's column-axis forward,
 * whose checks these are, in its order: FQ_ERR_DTYPE, FQ_ERR_ARG (unknown fmt, flag bits), FQ_ERR_SHAPE (negative or overflowing shape,
 * rows not a multiple of 32), 0 without a launch for an empty shape, FQ_ERR_NULL, FQ_ERR_ARG (y == x), FQ_ERR_UNSUPPORTED (x / y not
 * 16-byte aligned, cols * element size not a multiple of 16, more tiles than one launch's grid holds). */
int fqs_mx_fwd_cols(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, int flags, uint64_t seed, uint64_t stream_id, void* stream);

/* Host only, no HIP call: out[k] (HOST memory, n values) = R16 of flat element first + k of a tensor of `dtype`, computed on the host by
 * the function the kernels call on the device (the flat index -> counter and word selection included).  For tests of the 64-bit counter
 * and for callers that replay a launch's noise.  FQ_ERR_DTYPE, FQ_ERR_SHAPE (negative first / n, n above 2^24, first + n overflowing),
 * 0 for n == 0, FQ_ERR_NULL. */
int fqs_mx_noise(uint64_t seed, uint64_t stream_id, int64_t first, int64_t n, int dtype, uint16_t* out);

#ifdef __cplusplus
}
#endif
#endif /* LLMQAT_FAKEQUANT_SR_H */
