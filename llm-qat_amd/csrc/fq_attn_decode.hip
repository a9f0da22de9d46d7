// fq_attn_decode.hip -- the decode-attention kernels (fq_attn_decode.h) and their entry points (include/llmqat_fakequant_attn_decode.h): a
// translation unit of its own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_attn_decode.h"

#include "fq_attn_decode.h"

using namespace fq;

namespace {

struct DecShape {
    int64_t B, H, T, D, S, cus;
};

// the largest element offset of a [n0, n1, n2, D] view by strides fits 62 bits
bool span_ok(int64_t n0, int64_t s0, int64_t n1, int64_t s1, int64_t n2, int64_t s2, int64_t D) {
    const __int128 top = (__int128)(n0 - 1) * s0 + (__int128)(n1 - 1) * s1 + (__int128)(n2 - 1) * s2 + D;
    return top < ((__int128)1 << 62);
}

// the dtype and the shape refusals of both entry points, in the header's order: ROW_CONTINUE, or the refusal
int dec_dtype(int dtype) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16)
        return fail(FQ_ERR_DTYPE, "dtype code %d is not served by the decode attention: bfloat16 or float16 q, k, v", dtype);
    return ROW_CONTINUE;
}
int dec_shape(const DecShape& s) {
    if (s.B <= 0 || s.H <= 0 || s.S <= 0) return fail(FQ_ERR_SHAPE, "B=%lld H=%lld S=%lld must be positive", (long long)s.B, (long long)s.H, (long long)s.S);
    if (s.T < 1 || s.T > DEC_MAX_T) return fail(FQ_ERR_SHAPE, "T=%lld is not in 1 .. %d query rows", (long long)s.T, DEC_MAX_T);
    if (s.D != 64 && s.D != 128) return fail(FQ_ERR_SHAPE, "D=%lld is not a head size served (64, 128)", (long long)s.D);
    if (s.B > INT64_MAX / s.H || !span_ok(s.B * s.H, DEC_MAX_SPLIT * DEC_MAX_T * (s.D + 2) * 4, 1, 0, 1, 0, 0) || !span_ok(s.B * s.H, s.S, 1, 0, 1, 0, 0))
        return fail(FQ_ERR_SHAPE, "B * H * S overflows");
    return ROW_CONTINUE;
}

size_t dec_ws_bytes(const DecShape& s, int64_t nsplit) { return nsplit == 1 ? 0 : (size_t)(s.B * s.H * nsplit * s.T * (s.D + 2) * 4); }

bool strides_vec(const int64_t* st) { return st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0; }

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqd_attn_decode_workspace(int64_t B, int64_t H, int64_t T, int64_t D, int64_t S, int64_t cus, int dtype, size_t* bytes, int64_t* nsplit) {
    const DecShape s{B, H, T, D, S, cus};
    if (const int rc = dec_dtype(dtype); rc != ROW_CONTINUE) return rc;
    if (const int rc = dec_shape(s); rc != ROW_CONTINUE) return rc;
    if (!bytes || !nsplit) return fail(FQ_ERR_NULL, "bytes / nsplit must not be NULL");
    *nsplit = dec_nsplit(B * H, S, cus);
    *bytes = dec_ws_bytes(s, *nsplit);
    return ok();
}

FQ_API int fqd_attn_decode_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, void* workspace, size_t workspace_bytes,
                               int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb, int64_t v_sh,
                               int64_t v_st, int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H, int64_t T, int64_t S,
                               int64_t D, int64_t cus, float inv, int dtype, int mask_dtype, void* stream) {
    const DecShape s{B, H, T, D, S, cus};
    if (const int rc = dec_dtype(dtype); rc != ROW_CONTINUE) return rc;
    if (mask && (mask_dtype < 0 || mask_dtype > FQ_DTYPE_F64)) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", mask_dtype);
    if (mask && mask_dtype != dtype && mask_dtype != FQ_DTYPE_F32)
        return fail(FQ_ERR_DTYPE, "the dtype pair (q, k, v %d, mask %d) is not served: a mask in their dtype or in float32", dtype, mask_dtype);
    if (const int rc = dec_shape(s); rc != ROW_CONTINUE) return rc;
    const int64_t st[9] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st};
    for (const int64_t x : st)
        if (x < 0) return fail(FQ_ERR_SHAPE, "negative stride %lld", (long long)x);
    if (mask && (mask_batch_stride < 0 || mask_row_stride < 0))
        return fail(FQ_ERR_SHAPE, "negative mask stride (batch %lld, row %lld)", (long long)mask_batch_stride, (long long)mask_row_stride);
    if (!span_ok(B, q_sb, H, q_sh, T, q_st, D) || !span_ok(B, k_sb, H, k_sh, S, k_st, D) || !span_ok(B, v_sb, H, v_sh, S, v_st, D) ||
        (mask && !span_ok(B, mask_batch_stride, T, mask_row_stride, 1, 0, S)))
        return fail(FQ_ERR_SHAPE, "a tensor's extent overflows");
    if (!q || !k || !v || !out) return fail(FQ_ERR_NULL, "q / k / v / out must not be NULL");
    const void* ins[4] = {q, k, v, mask};
    for (const void* p : ins)
        if (p && (p == out || p == workspace)) return fail(FQ_ERR_ARG, "in-place (out or the workspace on an input) is not supported");
    if (workspace && workspace == out) return fail(FQ_ERR_ARG, "in-place (the workspace on out) is not supported");
    const int64_t nsplit = dec_nsplit(B * H, S, cus);
    const size_t need = dec_ws_bytes(s, nsplit);
    if (need && (!workspace || workspace_bytes < need))
        return fail(FQ_ERR_UNSUPPORTED, "workspace too small: %zu bytes, fqd_attn_decode_workspace asks for %zu", workspace ? workspace_bytes : (size_t)0, need);
    if (B * H > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "B * H = %lld exceeds one launch's grid", (long long)(B * H));

    DecArgs a{};
    a.q = q, a.k = k, a.v = v, a.mask = mask, a.out = out, a.ws = need ? (float*)workspace : nullptr;
    for (int i = 0; i < 3; ++i) a.qs[i] = st[i], a.ks[i] = st[3 + i], a.vs[i] = st[6 + i];
    a.mbs = mask_batch_stride, a.mrs = mask_row_stride;
    a.H = H, a.T = T, a.S = S, a.per = dec_chunk_tiles(B * H, S, cus), a.nsplit = (int)nsplit, a.inv = inv;
    const bool vec = aligned16(q) && aligned16(k) && aligned16(v) && strides_vec(a.qs) && strides_vec(a.ks) && strides_vec(a.vs);
    const int m_kind = !mask ? 0 : mask_dtype == dtype ? 1 : 2;
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    auto with = [&](auto sd, auto md, auto dd, auto vv) {
        constexpr int DT = decltype(sd)::value;
        launch_grid(dec_kernel<DT, decltype(md)::value, decltype(dd)::value, decltype(vv)::value != 0>, B * H, nsplit, DEC_WAVES * 64, stm, a);
        if (nsplit > 1) launch_grid(dec_combine_kernel<DT>, B * H, T, (int)D, stm, (const float*)a.ws, out, H, T, (int)D, (int)nsplit);
    };
    auto by_dt = [&](auto sd) {
        constexpr int DT = decltype(sd)::value;
        auto by_mask = [&](auto md) {
            if (D == 64) vec ? with(sd, md, Const<64>{}, Const<1>{}) : with(sd, md, Const<64>{}, Const<0>{});
            else vec ? with(sd, md, Const<128>{}, Const<1>{}) : with(sd, md, Const<128>{}, Const<0>{});
        };
        if (m_kind == 0) by_mask(Const<ATTN_NOMASK>{});
        else if (m_kind == 1) by_mask(Const<DT>{});
        else by_mask(Const<F32>{});
    };
    if (dtype == FQ_DTYPE_BF16) by_dt(Const<BF16>{});
    else by_dt(Const<F16>{});
    return launch_result();
}

}  // extern "C"
