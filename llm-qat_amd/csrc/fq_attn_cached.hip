// fq_attn_cached.hip -- the decode attention over an in-place K/V cache (fq_attn_cached.h) and its entry points
// (include/llmqat_fakequant_attn_cached.h): a translation unit of its own, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_attn_cached.h"

#include "fq_attn_cached.h"

using namespace fq;

namespace {

struct CacShape {
    int64_t B, H, Hkv, T, D, Smax, cus;
    int64_t G() const { return H / Hkv; }
    int64_t HP() const { return gqa_pack_heads(G(), T); }
    int64_t NP() const { return gqa_packs(G(), T); }
    int64_t wgs() const { return B * Hkv * NP(); }
    int64_t nsplit() const { return dec_nsplit(wgs(), Smax, cus); }
    size_t ws_bytes() const { return nsplit() == 1 ? 0 : (size_t)(wgs() * nsplit() * HP() * T * (D + 2) * 4); }
};

// a [B, n1, n2, D] view by strides: its extent in elements, 0 where that does not fit 62 bits
int64_t extent(int64_t B, const int64_t* st, int64_t n1, int64_t n2, int64_t D) {
    const __int128 top = (__int128)(B - 1) * st[0] + (__int128)(n1 - 1) * st[1] + (__int128)(n2 - 1) * st[2] + D;
    return top < ((__int128)1 << 62) ? (int64_t)top : 0;
}
bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {      // 16-bit elements
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + 2 * (uintptr_t)nb && pb < pa + 2 * (uintptr_t)na;
}
bool mult8(const int64_t* st) { return st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0; }

// the refusals both entry points share, in the header's order: ROW_CONTINUE, or the refusal
int cac_shape(const CacShape& s, int dtype) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16)
        return fail(FQ_ERR_DTYPE, "dtype code %d is not served by the cached decode attention: bfloat16 or float16", dtype);
    if (s.B <= 0 || s.H <= 0 || s.Smax <= 0)
        return fail(FQ_ERR_SHAPE, "B=%lld H=%lld Smax=%lld must be positive", (long long)s.B, (long long)s.H, (long long)s.Smax);
    if (s.Hkv < 1 || s.H % s.Hkv != 0) return fail(FQ_ERR_SHAPE, "Hkv=%lld K/V heads must be positive and divide H=%lld", (long long)s.Hkv, (long long)s.H);
    if (s.T < 1 || s.T > DEC_MAX_T) return fail(FQ_ERR_SHAPE, "T=%lld is not in 1 .. %d query rows", (long long)s.T, DEC_MAX_T);
    if (s.D != 64 && s.D != 128) return fail(FQ_ERR_SHAPE, "D=%lld is not a head size served (64, 128)", (long long)s.D);
    if (s.Smax > 0x7FFFFFFF - s.T) return fail(FQ_ERR_SHAPE, "Smax=%lld + T is beyond the int32 lengths' range", (long long)s.Smax);
    const int64_t row = DEC_MAX_SPLIT * DEC_MAX_T * (s.D + 2) * 4;      // the workspace of a (batch, head) is bounded by the ungrouped one's
    if (s.B > INT64_MAX / s.H || (__int128)(s.B * s.H) * row >= ((__int128)1 << 62) || (__int128)(s.B * s.H) * s.Smax >= ((__int128)1 << 62))
        return fail(FQ_ERR_SHAPE, "B * H * Smax overflows");
    return ROW_CONTINUE;
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqu_attn_cached_workspace(int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t D, int64_t Smax, int64_t cus, int dtype, size_t* bytes,
                                     int64_t* nsplit) {
    const CacShape s{B, H, Hkv, T, D, Smax, cus};
    if (const int rc = cac_shape(s, dtype); rc != ROW_CONTINUE) return rc;
    if (!bytes || !nsplit) return fail(FQ_ERR_NULL, "bytes / nsplit must not be NULL");
    *nsplit = s.nsplit();
    *bytes = s.ws_bytes();
    return ok();
}

FQ_API int fqu_attn_cached_fwd(const void* q, const void* k_new, const void* v_new, void* k_cache, void* v_cache, const int32_t* cache_lens,
                               const int32_t* cache_starts, void* out, void* workspace, size_t workspace_bytes, int64_t q_sb, int64_t q_sh,
                               int64_t q_st, int64_t kn_sb, int64_t kn_sh, int64_t kn_st, int64_t vn_sb, int64_t vn_sh, int64_t vn_st, int64_t kc_sb,
                               int64_t kc_sh, int64_t kc_st, int64_t vc_sb, int64_t vc_sh, int64_t vc_st, int64_t B, int64_t H, int64_t Hkv, int64_t T,
                               int64_t Smax, int64_t D, int64_t cus, float inv, int dtype, void* stream) {
    const CacShape s{B, H, Hkv, T, D, Smax, cus};
    if (const int rc = cac_shape(s, dtype); rc != ROW_CONTINUE) return rc;
    const int64_t st[15] = {q_sb, q_sh, q_st, kn_sb, kn_sh, kn_st, vn_sb, vn_sh, vn_st, kc_sb, kc_sh, kc_st, vc_sb, vc_sh, vc_st};
    for (const int64_t x : st)
        if (x < 0) return fail(FQ_ERR_SHAPE, "negative stride %lld", (long long)x);
    const int64_t nq = extent(B, st, H, T, D), nkn = extent(B, st + 3, Hkv, T, D), nvn = extent(B, st + 6, Hkv, T, D);
    const int64_t nkc = extent(B, st + 9, Hkv, Smax, D), nvc = extent(B, st + 12, Hkv, Smax, D);
    if (!nq || !nkn || !nvn || !nkc || !nvc) return fail(FQ_ERR_SHAPE, "a tensor's extent overflows");
    if (!q || !k_new || !v_new || !k_cache || !v_cache || !cache_lens || !out)
        return fail(FQ_ERR_NULL, "q / k_new / v_new / k_cache / v_cache / cache_lens / out must not be NULL");
    const void* reads[3] = {q, k_new, v_new};
    const int64_t nreads[3] = {nq, nkn, nvn};
    for (int i = 0; i < 3; ++i)
        if (overlap(reads[i], nreads[i], k_cache, nkc) || overlap(reads[i], nreads[i], v_cache, nvc))
            return fail(FQ_ERR_ARG, "q, k_new or v_new overlaps a cache: the append is in place and would race the reads");
    if (k_cache == v_cache) return fail(FQ_ERR_ARG, "k_cache and v_cache are one buffer");
    const void* others[7] = {q, k_new, v_new, k_cache, v_cache, cache_lens, cache_starts};
    for (const void* p : others)
        if (p && (p == out || p == workspace)) return fail(FQ_ERR_ARG, "in-place (out or the workspace on another argument) is not supported");
    if (workspace && workspace == out) return fail(FQ_ERR_ARG, "in-place (the workspace on out) is not supported");
    const int64_t nsplit = s.nsplit();
    const size_t need = s.ws_bytes();
    if (need && (!workspace || workspace_bytes < need))
        return fail(FQ_ERR_UNSUPPORTED, "workspace too small: %zu bytes, fqu_attn_cached_workspace asks for %zu", workspace ? workspace_bytes : (size_t)0, need);
    if (s.wgs() > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "B * Hkv * packs = %lld exceeds one launch's grid", (long long)s.wgs());

    CacArgs ca{};
    DecArgs& a = ca.d;
    a.q = q, a.out = out, a.ws = need ? (float*)workspace : nullptr, a.inv = inv;
    a.H = H, a.T = T, a.S = Smax, a.nsplit = (int)nsplit, a.Hkv = Hkv, a.G = s.G(), a.HP = s.HP(), a.NP = s.NP();
    ca.kn = k_new, ca.vn = v_new, ca.kc = k_cache, ca.vc = v_cache, ca.lens = cache_lens, ca.starts = cache_starts;
    for (int i = 0; i < 3; ++i) a.qs[i] = st[i], ca.kns[i] = st[3 + i], ca.vns[i] = st[6 + i], ca.kcs[i] = st[9 + i], ca.vcs[i] = st[12 + i];
    const bool vec = aligned16(q) && aligned16(k_new) && aligned16(v_new) && aligned16(k_cache) && aligned16(v_cache) && mult8(a.qs) &&
                     mult8(ca.kns) && mult8(ca.vns) && mult8(ca.kcs) && mult8(ca.vcs);
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    auto with = [&](auto sd, auto dd, auto vv) {
        constexpr int DT = decltype(sd)::value;
        launch_grid(cac_kernel<DT, decltype(dd)::value, decltype(vv)::value != 0>, s.wgs(), nsplit, DEC_WAVES * 64, stm, ca);
        if (nsplit > 1)
            launch_grid(gqa_combine_kernel<DT>, s.wgs(), a.HP * a.T, (int)D, stm, (const float*)a.ws, out, H, a.G, a.HP, a.NP, T, (int)D, (int)nsplit);
    };
    auto by_dt = [&](auto sd) {
        if (D == 64) vec ? with(sd, Const<64>{}, Const<1>{}) : with(sd, Const<64>{}, Const<0>{});
        else vec ? with(sd, Const<128>{}, Const<1>{}) : with(sd, Const<128>{}, Const<0>{});
    };
    if (dtype == FQ_DTYPE_BF16) by_dt(Const<BF16>{});
    else by_dt(Const<F16>{});
    return launch_result();
}

}  // extern "C"
