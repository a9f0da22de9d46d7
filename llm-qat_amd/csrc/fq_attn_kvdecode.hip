// fq_attn_kvdecode.hip -- the decode attention over a cache of integer codes (fq_attn_kvdecode.h) and its entry points
// (include/llmqat_fakequant_attn_kvdecode.h): a translation unit of its own, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_attn_kvdecode.h"

#include "fq_attn_kvdecode.h"

using namespace fq;

namespace {

struct KvdShape {
    int64_t B, H, T, D, S, cus;
};

// the largest element offset of a [n0, n1, n2, D] view by strides fits 62 bits
bool span_ok(int64_t n0, int64_t s0, int64_t n1, int64_t s1, int64_t n2, int64_t s2, int64_t D) {
    const __int128 top = (__int128)(n0 - 1) * s0 + (__int128)(n1 - 1) * s1 + (__int128)(n2 - 1) * s2 + D;
    return top < ((__int128)1 << 62);
}

// the refusals that both entry points share, in the header's order: ROW_CONTINUE, or the refusal
int kvd_dtype(int dtype) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16)
        return fail(FQ_ERR_DTYPE, "dtype code %d is not served by the decode attention: bfloat16 or float16 q", dtype);
    return ROW_CONTINUE;
}
int kvd_bits(int code_bits) {
    if (code_bits != 8 && code_bits != 4) return fail(FQ_ERR_BITS, "code_bits=%d is not a container served: 8 (int8) or 4 (packed int4)", code_bits);
    return ROW_CONTINUE;
}
int kvd_shape(const KvdShape& s) {
    if (s.B <= 0 || s.H <= 0 || s.S <= 0) return fail(FQ_ERR_SHAPE, "B=%lld H=%lld S=%lld must be positive", (long long)s.B, (long long)s.H, (long long)s.S);
    if (s.T < 1 || s.T > DEC_MAX_T) return fail(FQ_ERR_SHAPE, "T=%lld is not in 1 .. %d query rows", (long long)s.T, DEC_MAX_T);
    if (s.D != 64 && s.D != 128) return fail(FQ_ERR_SHAPE, "D=%lld is not a head size served (64, 128)", (long long)s.D);
    if (s.B > INT64_MAX / s.H || !span_ok(s.B * s.H, DEC_MAX_SPLIT * DEC_MAX_T * (s.D + 2) * 4, 1, 0, 1, 0, 0) || !span_ok(s.B * s.H, s.S, 1, 0, 1, 0, 0))
        return fail(FQ_ERR_SHAPE, "B * H * S overflows");
    return ROW_CONTINUE;
}

size_t kvd_ws_bytes(const KvdShape& s, int64_t nsplit) { return nsplit == 1 ? 0 : (size_t)(s.B * s.H * nsplit * s.T * (s.D + 2) * 4); }

bool mult(const int64_t* st, int64_t n) { return st[0] % n == 0 && st[1] % n == 0 && st[2] % n == 0; }

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqk_attn_kvdecode_workspace(int64_t B, int64_t H, int64_t T, int64_t D, int64_t S, int64_t cus, int dtype, int code_bits, size_t* bytes,
                                       int64_t* nsplit) {
    const KvdShape s{B, H, T, D, S, cus};
    if (const int rc = kvd_dtype(dtype); rc != ROW_CONTINUE) return rc;
    if (const int rc = kvd_bits(code_bits); rc != ROW_CONTINUE) return rc;
    if (const int rc = kvd_shape(s); rc != ROW_CONTINUE) return rc;
    if (!bytes || !nsplit) return fail(FQ_ERR_NULL, "bytes / nsplit must not be NULL");
    *nsplit = dec_nsplit(B * H, S, cus);
    *bytes = kvd_ws_bytes(s, *nsplit);
    return ok();
}

FQ_API int fqk_attn_kvdecode_fwd(const void* q, const void* k_codes, const float* k_t2, const void* v_codes, const float* v_t2, const void* mask,
                                 const void* cos, const void* sin, const int64_t* key_positions, void* out, void* workspace, size_t workspace_bytes,
                                 int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb, int64_t v_sh,
                                 int64_t v_st, int64_t k_t2_batch_stride, int64_t v_t2_batch_stride, int64_t mask_batch_stride, int64_t mask_row_stride,
                                 int64_t pos_batch_stride, int64_t P, int64_t B, int64_t H, int64_t T, int64_t S, int64_t D, int64_t cus, float inv,
                                 int dtype, int mask_dtype, int code_bits, void* stream) {
    const KvdShape s{B, H, T, D, S, cus};
    if (const int rc = kvd_dtype(dtype); rc != ROW_CONTINUE) return rc;
    if (mask && (mask_dtype < 0 || mask_dtype > FQ_DTYPE_F64)) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", mask_dtype);
    if (mask && mask_dtype != dtype && mask_dtype != FQ_DTYPE_F32)
        return fail(FQ_ERR_DTYPE, "the dtype pair (q %d, mask %d) is not served: a mask in q's dtype or in float32", dtype, mask_dtype);
    if (const int rc = kvd_bits(code_bits); rc != ROW_CONTINUE) return rc;
    if (const int rc = kvd_shape(s); rc != ROW_CONTINUE) return rc;
    const int64_t st[9] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st};
    for (const int64_t x : st)
        if (x < 0) return fail(FQ_ERR_SHAPE, "negative stride %lld", (long long)x);
    if (k_t2_batch_stride < 0 || v_t2_batch_stride < 0 || (key_positions && pos_batch_stride < 0))
        return fail(FQ_ERR_SHAPE, "negative stride of t2 (%lld, %lld) or of the positions (%lld)", (long long)k_t2_batch_stride, (long long)v_t2_batch_stride,
                    (long long)pos_batch_stride);
    if (mask && (mask_batch_stride < 0 || mask_row_stride < 0))
        return fail(FQ_ERR_SHAPE, "negative mask stride (batch %lld, row %lld)", (long long)mask_batch_stride, (long long)mask_row_stride);
    if (cos && (P <= 0 || !span_ok(P, D, 1, 0, 1, 0, D))) return fail(FQ_ERR_SHAPE, "P=%lld table rows must be positive", (long long)P);
    const int64_t cd = D * code_bits / 8;      // bytes of a key's codes
    if (!span_ok(B, q_sb, H, q_sh, T, q_st, D) || !span_ok(B, k_sb, H, k_sh, S, k_st, cd) || !span_ok(B, v_sb, H, v_sh, S, v_st, cd) ||
        !span_ok(B, k_t2_batch_stride, 1, 0, 1, 0, S) || !span_ok(B, v_t2_batch_stride, 1, 0, 1, 0, S) ||
        (key_positions && !span_ok(B, pos_batch_stride, 1, 0, 1, 0, S)) || (mask && !span_ok(B, mask_batch_stride, T, mask_row_stride, 1, 0, S)))
        return fail(FQ_ERR_SHAPE, "a tensor's extent overflows");
    if (!q || !k_codes || !k_t2 || !v_codes || !v_t2 || !out) return fail(FQ_ERR_NULL, "q / k_codes / k_t2 / v_codes / v_t2 / out must not be NULL");
    if ((cos == nullptr) != (sin == nullptr)) return fail(FQ_ERR_NULL, "cos and sin come together or not at all");
    if (key_positions && !cos) return fail(FQ_ERR_NULL, "key_positions without the tables");
    const void* ins[9] = {q, k_codes, k_t2, v_codes, v_t2, mask, cos, sin, key_positions};
    for (const void* p : ins)
        if (p && (p == out || p == workspace)) return fail(FQ_ERR_ARG, "in-place (out or the workspace on an input) is not supported");
    if (workspace && workspace == out) return fail(FQ_ERR_ARG, "in-place (the workspace on out) is not supported");
    const int64_t nsplit = dec_nsplit(B * H, S, cus);
    const size_t need = kvd_ws_bytes(s, nsplit);
    if (need && (!workspace || workspace_bytes < need))
        return fail(FQ_ERR_UNSUPPORTED, "workspace too small: %zu bytes, fqk_attn_kvdecode_workspace asks for %zu", workspace ? workspace_bytes : (size_t)0, need);
    if (B * H > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "B * H = %lld exceeds one launch's grid", (long long)(B * H));

    KvdArgs ka{};
    DecArgs& a = ka.d;
    a.q = q, a.k = k_codes, a.v = v_codes, a.mask = mask, a.out = out, a.ws = need ? (float*)workspace : nullptr;
    for (int i = 0; i < 3; ++i) a.qs[i] = st[i], a.ks[i] = st[3 + i], a.vs[i] = st[6 + i];
    a.mbs = mask_batch_stride, a.mrs = mask_row_stride;
    a.H = H, a.T = T, a.S = S, a.per = dec_chunk_tiles(B * H, S, cus), a.nsplit = (int)nsplit, a.inv = inv;
    ka.kt2 = k_t2, ka.vt2 = v_t2, ka.kt2_bs = k_t2_batch_stride, ka.vt2_bs = v_t2_batch_stride;
    ka.cos = cos, ka.sin = sin, ka.pos = key_positions, ka.pos_bs = key_positions ? pos_batch_stride : 0, ka.P = P;
    const bool vec = aligned16(q) && aligned16(k_codes) && aligned16(v_codes) && mult(a.qs, 8) && mult(a.ks, 16) && mult(a.vs, 16) &&
                     (!cos || (aligned16(cos) && aligned16(sin)));
    const int m_kind = !mask ? 0 : mask_dtype == dtype ? 1 : 2;
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    auto with = [&](auto sd, auto md, auto dd, auto cb, auto rot, auto vv) {
        constexpr int DT = decltype(sd)::value;
        launch_grid(kvd_kernel<DT, decltype(md)::value, decltype(dd)::value, decltype(cb)::value, decltype(rot)::value != 0, decltype(vv)::value != 0>, B * H,
                    nsplit, DEC_WAVES * 64, stm, ka);
        if (nsplit > 1) launch_grid(dec_combine_kernel<DT>, B * H, T, (int)D, stm, (const float*)a.ws, out, H, T, (int)D, (int)nsplit);
    };
    auto by_dt = [&](auto sd) {
        constexpr int DT = decltype(sd)::value;
        auto by_mask = [&](auto md) {
            auto by_d = [&](auto dd) {
                auto by_cb = [&](auto cb) {
                    auto by_rot = [&](auto rot) { vec ? with(sd, md, dd, cb, rot, Const<1>{}) : with(sd, md, dd, cb, rot, Const<0>{}); };
                    cos ? by_rot(Const<1>{}) : by_rot(Const<0>{});
                };
                code_bits == 8 ? by_cb(Const<8>{}) : by_cb(Const<4>{});
            };
            D == 64 ? by_d(Const<64>{}) : by_d(Const<128>{});
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
