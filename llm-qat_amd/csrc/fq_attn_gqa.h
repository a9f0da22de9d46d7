// fq_attn_gqa.h -- grouped-query attention: the kernels behind include/llmqat_fakequant_attn_gqa.h.
//
// k and v (or their codes) are [B, Hkv, S, D] with H = G Hkv query heads; query head h reads K/V head h / G.
//
// Decode.  The T <= 16 query rows of one head fill T of the 16 columns of both matrix instructions.  Here the columns are shared by
// HP = min(G, 16 / T) heads of one group: a workgroup serves one (batch, K/V head, pack of HP heads), grid (B Hkv NP, nsplit) with
// NP = ceil(G / HP), and column j is token j % T of head hkv G + pack HP + j / T (dec_column).  The K fragments, the V stage, the
// divisors, the positions, the rotary tables and, in the codes kernel, the dequantisation and rotation of K are per key: they are
// loaded and computed once for the pack.  What depends on the column is q, the mask row and the address of the result.  The kernels are
// dec_body / kvd_body under that column map: per column the arithmetic is the ungrouped kernels', to the bit where S is one chunk
// either way.  The split along S is asked with B Hkv NP workgroups, so fewer workgroups cut S into more chunks; the workspace is
// [B Hkv NP, nsplit, HP T, D + 2] and gqa_combine_kernel merges the chunks of every live column in chunk order.  No atomics.
//
// Prefill.  pre_kernel with K and V of head h / G (its GQA instantiations); no packing: a workgroup's 128 query rows fill the columns.
#pragma once
#include "fq_attn_kvdecode.h"
#include "fq_attn_prefill.h"

namespace fq {

// heads of a pack, packs of a K/V head
inline int64_t gqa_pack_heads(int64_t G, int64_t T) { return G < DEC_MAX_T / T ? G : DEC_MAX_T / T; }
inline int64_t gqa_packs(int64_t G, int64_t T) {
    const int64_t hp = gqa_pack_heads(G, T);
    return (G + hp - 1) / hp;
}

template <int DT, int MDT, int D, bool VEC> __global__ __launch_bounds__(DEC_WAVES * 64) void gqa_dec_kernel(DecArgs a) { dec_body<DT, MDT, D, VEC, true>(a); }

template <int DT, int MDT, int D, int CB, bool ROT, bool VEC>
__global__ __launch_bounds__(DEC_WAVES * 64) void gqa_kvd_kernel(KvdArgs ka) { kvd_body<DT, MDT, D, CB, ROT, VEC, true>(ka); }

// the chunks of one column into out, in chunk order: grid (B Hkv NP, HP T), D threads; a dead column's block leaves at once
template <int DT>
__global__ __launch_bounds__(128) void gqa_combine_kernel(const float* ws, void* out, int64_t H, int64_t G, int64_t HP, int64_t NP, int64_t T, int D, int nsplit) {
    const int64_t x = blockIdx.x, per = (H / G) * NP, b = x / per, r = x % per;
    const int64_t j = blockIdx.y, hl = (r % NP) * HP + j / T, t = j % T;
    if (hl >= G) return;
    const int64_t h = (r / NP) * G + hl;
    const int64_t row = D + 2, step = HP * T * row;
    dec_combine<DT>(ws + (x * nsplit * HP * T + j) * row, step, out, ((b * T + t) * H + h) * D, nsplit);
}

}  // namespace fq
