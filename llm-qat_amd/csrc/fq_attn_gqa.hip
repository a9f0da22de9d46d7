// fq_attn_gqa.hip -- the grouped-query attention kernels (fq_attn_gqa.h) and their entry points (include/llmqat_fakequant_attn_gqa.h): a
// translation unit of its own, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_attn_gqa.h"

#include "fq_attn_gqa.h"

using namespace fq;

namespace {

struct GqaShape {
    int64_t B, H, Hkv, T, D, S, cus;
    int64_t G() const { return H / Hkv; }
    int64_t HP() const { return gqa_pack_heads(G(), T); }
    int64_t NP() const { return gqa_packs(G(), T); }
    int64_t wgs() const { return B * Hkv * NP(); }      // workgroups of a chunk
};

// the largest element offset of a [n0, n1, n2, D] view by strides fits 62 bits
bool span_ok(int64_t n0, int64_t s0, int64_t n1, int64_t s1, int64_t n2, int64_t s2, int64_t D) {
    const __int128 top = (__int128)(n0 - 1) * s0 + (__int128)(n1 - 1) * s1 + (__int128)(n2 - 1) * s2 + D;
    return top < ((__int128)1 << 62);
}
bool mult(const int64_t* st, int64_t n) { return st[0] % n == 0 && st[1] % n == 0 && st[2] % n == 0; }

// the refusals the entry points share, in the header's order: ROW_CONTINUE, or the refusal
int gqa_dtype(int dtype, const char* what) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16) return fail(FQ_ERR_DTYPE, "dtype code %d is not served by the %s attention: bfloat16 or float16", dtype, what);
    return ROW_CONTINUE;
}
int gqa_mask_dtype(const void* mask, int dtype, int mask_dtype) {
    if (mask && (mask_dtype < 0 || mask_dtype > FQ_DTYPE_F64)) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", mask_dtype);
    if (mask && mask_dtype != dtype && mask_dtype != FQ_DTYPE_F32)
        return fail(FQ_ERR_DTYPE, "the dtype pair (q %d, mask %d) is not served: a mask in q's dtype or in float32", dtype, mask_dtype);
    return ROW_CONTINUE;
}
int gqa_bits(int code_bits) {
    if (code_bits != 8 && code_bits != 4) return fail(FQ_ERR_BITS, "code_bits=%d is not a container served: 8 (int8) or 4 (packed int4)", code_bits);
    return ROW_CONTINUE;
}
int gqa_heads(int64_t H, int64_t Hkv) {
    if (Hkv < 1 || H % Hkv != 0) return fail(FQ_ERR_SHAPE, "Hkv=%lld K/V heads must be positive and divide H=%lld", (long long)Hkv, (long long)H);
    return ROW_CONTINUE;
}
int gqa_dec_shape(const GqaShape& s) {
    if (s.B <= 0 || s.H <= 0 || s.S <= 0) return fail(FQ_ERR_SHAPE, "B=%lld H=%lld S=%lld must be positive", (long long)s.B, (long long)s.H, (long long)s.S);
    if (const int rc = gqa_heads(s.H, s.Hkv); rc != ROW_CONTINUE) return rc;
    if (s.T < 1 || s.T > DEC_MAX_T) return fail(FQ_ERR_SHAPE, "T=%lld is not in 1 .. %d query rows", (long long)s.T, DEC_MAX_T);
    if (s.D != 64 && s.D != 128) return fail(FQ_ERR_SHAPE, "D=%lld is not a head size served (64, 128)", (long long)s.D);
    // a pack's HP T <= 16 columns and NP <= G: the workspace of B Hkv NP workgroups is bounded by the ungrouped one's
    if (s.B > INT64_MAX / s.H || !span_ok(s.B * s.H, DEC_MAX_SPLIT * DEC_MAX_T * (s.D + 2) * 4, 1, 0, 1, 0, 0) || !span_ok(s.B * s.H, s.S, 1, 0, 1, 0, 0))
        return fail(FQ_ERR_SHAPE, "B * H * S overflows");
    return ROW_CONTINUE;
}
int gqa_strides(const int64_t (&st)[9], const void* mask, int64_t mbs, int64_t mrs) {
    for (const int64_t x : st)
        if (x < 0) return fail(FQ_ERR_SHAPE, "negative stride %lld", (long long)x);
    if (mask && (mbs < 0 || mrs < 0)) return fail(FQ_ERR_SHAPE, "negative mask stride (batch %lld, row %lld)", (long long)mbs, (long long)mrs);
    return ROW_CONTINUE;
}

int64_t gqa_nsplit(const GqaShape& s) { return dec_nsplit(s.wgs(), s.S, s.cus); }
size_t gqa_ws_bytes(const GqaShape& s, int64_t nsplit) { return nsplit == 1 ? 0 : (size_t)(s.wgs() * nsplit * s.HP() * s.T * (s.D + 2) * 4); }

int gqa_workspace(const GqaShape& s, size_t* bytes, int64_t* nsplit) {
    if (const int rc = gqa_dec_shape(s); rc != ROW_CONTINUE) return rc;
    if (!bytes || !nsplit) return fail(FQ_ERR_NULL, "bytes / nsplit must not be NULL");
    *nsplit = gqa_nsplit(s);
    *bytes = gqa_ws_bytes(s, *nsplit);
    return ok();
}
// the refusals behind the pointers: the workspace and the grid; -> nsplit through *n
int gqa_launch_ok(const GqaShape& s, const void* workspace, size_t workspace_bytes, const char* query, int64_t* n) {
    *n = gqa_nsplit(s);
    const size_t need = gqa_ws_bytes(s, *n);
    if (need && (!workspace || workspace_bytes < need))
        return fail(FQ_ERR_UNSUPPORTED, "workspace too small: %zu bytes, %s asks for %zu", workspace ? workspace_bytes : (size_t)0, query, need);
    if (s.wgs() > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "B * Hkv * packs = %lld exceeds one launch's grid", (long long)s.wgs());
    return ROW_CONTINUE;
}
void gqa_fill(DecArgs& a, const GqaShape& s, const int64_t (&st)[9], int64_t nsplit) {
    for (int i = 0; i < 3; ++i) a.qs[i] = st[i], a.ks[i] = st[3 + i], a.vs[i] = st[6 + i];
    a.H = s.H, a.T = s.T, a.S = s.S, a.per = dec_chunk_tiles(s.wgs(), s.S, s.cus), a.nsplit = (int)nsplit;
    a.Hkv = s.Hkv, a.G = s.G(), a.HP = s.HP(), a.NP = s.NP();
}
template <int DT> void gqa_combine(const DecArgs& a, const GqaShape& s, hipStream_t stm) {
    if (a.nsplit > 1)
        launch_grid(gqa_combine_kernel<DT>, s.wgs(), a.HP * a.T, (int)s.D, stm, (const float*)a.ws, a.out, a.H, a.G, a.HP, a.NP, a.T, (int)s.D, a.nsplit);
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqh_attn_decode_workspace(int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t D, int64_t S, int64_t cus, int dtype, size_t* bytes, int64_t* nsplit) {
    if (const int rc = gqa_dtype(dtype, "decode"); rc != ROW_CONTINUE) return rc;
    return gqa_workspace(GqaShape{B, H, Hkv, T, D, S, cus}, bytes, nsplit);
}

FQ_API int fqh_attn_decode_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, void* workspace, size_t workspace_bytes,
                               int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb, int64_t v_sh,
                               int64_t v_st, int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H, int64_t Hkv, int64_t T,
                               int64_t S, int64_t D, int64_t cus, float inv, int dtype, int mask_dtype, void* stream) {
    const GqaShape s{B, H, Hkv, T, D, S, cus};
    if (const int rc = gqa_dtype(dtype, "decode"); rc != ROW_CONTINUE) return rc;
    if (const int rc = gqa_mask_dtype(mask, dtype, mask_dtype); rc != ROW_CONTINUE) return rc;
    if (const int rc = gqa_dec_shape(s); rc != ROW_CONTINUE) return rc;
    const int64_t st[9] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st};
    if (const int rc = gqa_strides(st, mask, mask_batch_stride, mask_row_stride); rc != ROW_CONTINUE) return rc;
    if (!span_ok(B, q_sb, H, q_sh, T, q_st, D) || !span_ok(B, k_sb, Hkv, k_sh, S, k_st, D) || !span_ok(B, v_sb, Hkv, v_sh, S, v_st, D) ||
        (mask && !span_ok(B, mask_batch_stride, T, mask_row_stride, 1, 0, S)))
        return fail(FQ_ERR_SHAPE, "a tensor's extent overflows");
    if (!q || !k || !v || !out) return fail(FQ_ERR_NULL, "q / k / v / out must not be NULL");
    const void* ins[4] = {q, k, v, mask};
    for (const void* p : ins)
        if (p && (p == out || p == workspace)) return fail(FQ_ERR_ARG, "in-place (out or the workspace on an input) is not supported");
    if (workspace && workspace == out) return fail(FQ_ERR_ARG, "in-place (the workspace on out) is not supported");
    int64_t nsplit;
    if (const int rc = gqa_launch_ok(s, workspace, workspace_bytes, "fqh_attn_decode_workspace", &nsplit); rc != ROW_CONTINUE) return rc;

    DecArgs a{};
    a.q = q, a.k = k, a.v = v, a.mask = mask, a.out = out, a.ws = nsplit > 1 ? (float*)workspace : nullptr;
    a.mbs = mask_batch_stride, a.mrs = mask_row_stride, a.inv = inv;
    gqa_fill(a, s, st, nsplit);
    const bool vec = aligned16(q) && aligned16(k) && aligned16(v) && mult(a.qs, 8) && mult(a.ks, 8) && mult(a.vs, 8);
    const int m_kind = !mask ? 0 : mask_dtype == dtype ? 1 : 2;
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    auto with = [&](auto sd, auto md, auto dd, auto vv) {
        constexpr int DT = decltype(sd)::value;
        launch_grid(gqa_dec_kernel<DT, decltype(md)::value, decltype(dd)::value, decltype(vv)::value != 0>, s.wgs(), nsplit, DEC_WAVES * 64, stm, a);
        gqa_combine<DT>(a, s, stm);
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

FQ_API int fqh_attn_kvdecode_workspace(int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t D, int64_t S, int64_t cus, int dtype, int code_bits,
                                       size_t* bytes, int64_t* nsplit) {
    if (const int rc = gqa_dtype(dtype, "decode"); rc != ROW_CONTINUE) return rc;
    if (const int rc = gqa_bits(code_bits); rc != ROW_CONTINUE) return rc;
    return gqa_workspace(GqaShape{B, H, Hkv, T, D, S, cus}, bytes, nsplit);
}

FQ_API int fqh_attn_kvdecode_fwd(const void* q, const void* k_codes, const float* k_t2, const void* v_codes, const float* v_t2, const void* mask,
                                 const void* cos, const void* sin, const int64_t* key_positions, void* out, void* workspace, size_t workspace_bytes,
                                 int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb, int64_t v_sh,
                                 int64_t v_st, int64_t k_t2_batch_stride, int64_t v_t2_batch_stride, int64_t mask_batch_stride, int64_t mask_row_stride,
                                 int64_t pos_batch_stride, int64_t P, int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t S, int64_t D, int64_t cus,
                                 float inv, int dtype, int mask_dtype, int code_bits, void* stream) {
    const GqaShape s{B, H, Hkv, T, D, S, cus};
    if (const int rc = gqa_dtype(dtype, "decode"); rc != ROW_CONTINUE) return rc;
    if (const int rc = gqa_mask_dtype(mask, dtype, mask_dtype); rc != ROW_CONTINUE) return rc;
    if (const int rc = gqa_bits(code_bits); rc != ROW_CONTINUE) return rc;
    if (const int rc = gqa_dec_shape(s); rc != ROW_CONTINUE) return rc;
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
    if (!span_ok(B, q_sb, H, q_sh, T, q_st, D) || !span_ok(B, k_sb, Hkv, k_sh, S, k_st, cd) || !span_ok(B, v_sb, Hkv, v_sh, S, v_st, cd) ||
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
    int64_t nsplit;
    if (const int rc = gqa_launch_ok(s, workspace, workspace_bytes, "fqh_attn_kvdecode_workspace", &nsplit); rc != ROW_CONTINUE) return rc;

    KvdArgs ka{};
    DecArgs& a = ka.d;
    a.q = q, a.k = k_codes, a.v = v_codes, a.mask = mask, a.out = out, a.ws = nsplit > 1 ? (float*)workspace : nullptr;
    a.mbs = mask_batch_stride, a.mrs = mask_row_stride, a.inv = inv;
    gqa_fill(a, s, st, nsplit);
    ka.kt2 = k_t2, ka.vt2 = v_t2, ka.kt2_bs = k_t2_batch_stride, ka.vt2_bs = v_t2_batch_stride;
    ka.cos = cos, ka.sin = sin, ka.pos = key_positions, ka.pos_bs = key_positions ? pos_batch_stride : 0, ka.P = P;
    const bool vec = aligned16(q) && aligned16(k_codes) && aligned16(v_codes) && mult(a.qs, 8) && mult(a.ks, 16) && mult(a.vs, 16) &&
                     (!cos || (aligned16(cos) && aligned16(sin)));
    const int m_kind = !mask ? 0 : mask_dtype == dtype ? 1 : 2;
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    auto with = [&](auto sd, auto md, auto dd, auto cb, auto rot, auto vv) {
        constexpr int DT = decltype(sd)::value;
        launch_grid(gqa_kvd_kernel<DT, decltype(md)::value, decltype(dd)::value, decltype(cb)::value, decltype(rot)::value != 0, decltype(vv)::value != 0>,
                    s.wgs(), nsplit, DEC_WAVES * 64, stm, ka);
        gqa_combine<DT>(a, s, stm);
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

FQ_API int fqh_attn_prefill_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, int64_t q_sb, int64_t q_sh,
                                int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb, int64_t v_sh, int64_t v_st,
                                int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t S,
                                int64_t D, float inv, int dtype, int mask_dtype, int causal, void* stream) {
    if (const int rc = gqa_dtype(dtype, "prefill"); rc != ROW_CONTINUE) return rc;
    if (const int rc = gqa_mask_dtype(mask, dtype, mask_dtype); rc != ROW_CONTINUE) return rc;
    if (B <= 0 || H <= 0 || T <= 0 || S <= 0)
        return fail(FQ_ERR_SHAPE, "B=%lld H=%lld T=%lld S=%lld must be positive", (long long)B, (long long)H, (long long)T, (long long)S);
    if (const int rc = gqa_heads(H, Hkv); rc != ROW_CONTINUE) return rc;
    if (D != 64 && D != 128) return fail(FQ_ERR_SHAPE, "D=%lld is not a head size served (64, 128)", (long long)D);
    const int64_t st[9] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st};
    if (const int rc = gqa_strides(st, mask, mask_batch_stride, mask_row_stride); rc != ROW_CONTINUE) return rc;
    if (B > INT64_MAX / H || (__int128)(B * H) * T * D >= ((__int128)1 << 62)) return fail(FQ_ERR_SHAPE, "B * H * T * D overflows");      // out's extent
    if (!span_ok(B, q_sb, H, q_sh, T, q_st, D) || !span_ok(B, k_sb, Hkv, k_sh, S, k_st, D) || !span_ok(B, v_sb, Hkv, v_sh, S, v_st, D) ||
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
    a.H = H, a.T = T, a.S = S, a.inv = inv, a.G = H / Hkv;
    const bool vec = aligned16(q) && aligned16(k) && aligned16(v) && mult(a.qs, 8) && mult(a.ks, 8) && mult(a.vs, 8);
    const int m_kind = causal ? 3 : !mask ? 0 : mask_dtype == dtype ? 1 : 2;
    const uintptr_t m_align = m_kind == 2 ? 15u : 7u;
    const bool mvec = mask && (reinterpret_cast<uintptr_t>(mask) & m_align) == 0 && a.mbs % 4 == 0 && a.mrs % 4 == 0;
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    auto with = [&](auto sd, auto md, auto cz, auto dd, auto vv, auto mv) {
        launch_grid(pre_kernel<decltype(sd)::value, decltype(md)::value, decltype(cz)::value != 0, decltype(dd)::value, PRE_RPW / 16,
                               decltype(vv)::value != 0, decltype(mv)::value != 0, false, true>,
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
