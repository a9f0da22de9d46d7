// fq_attn_prefill.hip -- the prefill-attention kernel (fq_attn_prefill.h) and its entry point (include/llmqat_fakequant_attn_prefill.h): a
// translation unit of its own, entry point included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_attn_prefill.h"

#include "fq_attn_prefill.h"

using namespace fq;

namespace {

// the largest element offset of a [n0, n1, n2, D] view by strides fits 62 bits
bool span_ok(int64_t n0, int64_t s0, int64_t n1, int64_t s1, int64_t n2, int64_t s2, int64_t D) {
    const __int128 top = (__int128)(n0 - 1) * s0 + (__int128)(n1 - 1) * s1 + (__int128)(n2 - 1) * s2 + D;
    return top < ((__int128)1 << 62);
}

bool strides_vec(const int64_t* st) { return st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0; }

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqp_attn_prefill_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, int64_t q_sb, int64_t q_sh,
                                int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb, int64_t v_sh, int64_t v_st,
                                int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H, int64_t T, int64_t S, int64_t D,
                                float inv, int dtype, int mask_dtype, int causal, void* stream) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16)
        return fail(FQ_ERR_DTYPE, "dtype code %d is not served by the prefill attention: bfloat16 or float16 q, k, v", dtype);
    if (mask && (mask_dtype < 0 || mask_dtype > FQ_DTYPE_F64)) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", mask_dtype);
    if (mask && mask_dtype != dtype && mask_dtype != FQ_DTYPE_F32)
        return fail(FQ_ERR_DTYPE, "the dtype pair (q, k, v %d, mask %d) is not served: a mask in their dtype or in float32", dtype, mask_dtype);
    if (B <= 0 || H <= 0 || T <= 0 || S <= 0)
        return fail(FQ_ERR_SHAPE, "B=%lld H=%lld T=%lld S=%lld must be positive", (long long)B, (long long)H, (long long)T, (long long)S);
    if (D != 64 && D != 128) return fail(FQ_ERR_SHAPE, "D=%lld is not a head size served (64, 128)", (long long)D);
    const int64_t st[9] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st};
    for (const int64_t x : st)
        if (x < 0) return fail(FQ_ERR_SHAPE, "negative stride %lld", (long long)x);
    if (mask && (mask_batch_stride < 0 || mask_row_stride < 0))
        return fail(FQ_ERR_SHAPE, "negative mask stride (batch %lld, row %lld)", (long long)mask_batch_stride, (long long)mask_row_stride);
    if (B > INT64_MAX / H || (__int128)(B * H) * T * D >= ((__int128)1 << 62)) return fail(FQ_ERR_SHAPE, "B * H * T * D overflows");      // out's extent
    if (!span_ok(B, q_sb, H, q_sh, T, q_st, D) || !span_ok(B, k_sb, H, k_sh, S, k_st, D) || !span_ok(B, v_sb, H, v_sh, S, v_st, D) ||
        (mask && !span_ok(B, mask_batch_stride, T, mask_row_stride, 1, 0, S)))
        return fail(FQ_ERR_SHAPE, "a tensor's extent overflows");
    if (causal && T > S) return fail(FQ_ERR_SHAPE, "causal: T=%lld query rows are the last of S=%lld keys, so T <= S", (long long)T, (long long)S);
    if (!q || !k || !v || !out) return fail(FQ_ERR_NULL, "q / k / v / out must not be NULL");
    const void* ins[4] = {q, k, v, mask};
    for (const void* p : ins)
        if (p && p == out) return fail(FQ_ERR_ARG, "in-place (out on an input) is not supported");
    if (causal && mask) return fail(FQ_ERR_ARG, "causal together with a mask: give one of them");
    const int64_t nqt = pre_query_tiles(T);
    if (B * H > PRE_MAX_GRID_Y || nqt > 0x7FFFFFFF)
        return fail(FQ_ERR_UNSUPPORTED, "B * H = %lld or %lld query tiles exceed one launch's grid", (long long)(B * H), (long long)nqt);

    PreArgs a{};
    a.q = q, a.k = k, a.v = v, a.mask = mask, a.out = out;
    for (int i = 0; i < 3; ++i) a.qs[i] = st[i], a.ks[i] = st[3 + i], a.vs[i] = st[6 + i];
    a.mbs = mask ? mask_batch_stride : 0, a.mrs = mask ? mask_row_stride : 0;
    a.H = H, a.T = T, a.S = S, a.inv = inv;
    const bool vec = aligned16(q) && aligned16(k) && aligned16(v) && strides_vec(a.qs) && strides_vec(a.ks) && strides_vec(a.vs);
    const int m_kind = causal ? 3 : !mask ? 0 : mask_dtype == dtype ? 1 : 2;
    const uintptr_t m_align = m_kind == 2 ? 15u : 7u;
    const bool mvec = mask && (reinterpret_cast<uintptr_t>(mask) & m_align) == 0 && a.mbs % 4 == 0 && a.mrs % 4 == 0;
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    auto with = [&](auto sd, auto md, auto cz, auto dd, auto vv, auto mv) {
        launch_grid(pre_kernel<decltype(sd)::value, decltype(md)::value, decltype(cz)::value != 0, decltype(dd)::value, PRE_RPW / 16,
                               decltype(vv)::value != 0, decltype(mv)::value != 0>,
                    nqt, B * H, PRE_WAVES * 64, stm, a);
    };
    auto by_dt = [&](auto sd) {
        constexpr int DT = decltype(sd)::value;
        auto by_d = [&](auto md, auto cz, auto mv) {
            if (D == 64) vec ? with(sd, md, cz, Const<64>{}, Const<1>{}, mv) : with(sd, md, cz, Const<64>{}, Const<0>{}, mv);
            else vec ? with(sd, md, cz, Const<128>{}, Const<1>{}, mv) : with(sd, md, cz, Const<128>{}, Const<0>{}, mv);
        };
        if (m_kind == 0) by_d(Const<ATTN_NOMASK>{}, Const<0>{}, Const<0>{});
        else if (m_kind == 3) by_d(Const<ATTN_NOMASK>{}, Const<1>{}, Const<0>{});
        else if (m_kind == 1) mvec ? by_d(Const<DT>{}, Const<0>{}, Const<1>{}) : by_d(Const<DT>{}, Const<0>{}, Const<0>{});
        else mvec ? by_d(Const<F32>{}, Const<0>{}, Const<1>{}) : by_d(Const<F32>{}, Const<0>{}, Const<0>{});
    };
    if (dtype == FQ_DTYPE_BF16) by_dt(Const<BF16>{});
    else by_dt(Const<F16>{});
    return launch_result();
}

}  // extern "C"
