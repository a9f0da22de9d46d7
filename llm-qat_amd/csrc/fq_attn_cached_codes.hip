// fq_attn_cached_codes.hip -- the decode attention over an in-place K/V cache of integer codes (fq_attn_cached_codes.h) and its entry
// points (include/llmqat_fakequant_attn_cached_codes.h): a translation unit of its own, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_attn_cached_codes.h"

#include "fq_attn_cached_codes.h"

using namespace fq;

namespace {

struct CccShape {
    int64_t B, H, Hkv, T, D, Smax, cus;
    int64_t G() const { return H / Hkv; }
    int64_t HP() const { return gqa_pack_heads(G(), T); }
    int64_t NP() const { return gqa_packs(G(), T); }
    int64_t wgs() const { return B * Hkv * NP(); }
    int64_t nsplit() const { return dec_nsplit(wgs(), Smax, cus); }
    size_t ws_bytes() const { return nsplit() == 1 ? 0 : (size_t)(wgs() * nsplit() * HP() * T * (D + 2) * 4); }
};

// a [B, n1, n2, row] view by strides, in the strides' unit: its extent, 0 where that does not fit 60 bits
int64_t extent(int64_t B, const int64_t* st, int64_t n1, int64_t n2, int64_t row) {
    const __int128 top = (__int128)(B - 1) * st[0] + (__int128)(n1 - 1) * st[1] + (__int128)(n2 - 1) * st[2] + row;
    return top < ((__int128)1 << 60) ? (int64_t)top : 0;
}
struct Range {      // bytes
    const void* p;
    int64_t n;
};
bool overlap(const Range& a, const Range& b) {
    const uintptr_t pa = (uintptr_t)a.p, pb = (uintptr_t)b.p;
    return pa < pb + (uintptr_t)b.n && pb < pa + (uintptr_t)a.n;
}
bool mult(const int64_t* st, int64_t n) { return st[0] % n == 0 && st[1] % n == 0 && st[2] % n == 0; }

// the refusals both entry points share, in the header's order: ROW_CONTINUE, or the refusal
int ccc_shape(const CccShape& s, int dtype, int code_bits) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16)
        return fail(FQ_ERR_DTYPE, "dtype code %d is not served by the cached codes decode attention: bfloat16 or float16 q", dtype);
    if (code_bits != 8 && code_bits != 4) return fail(FQ_ERR_BITS, "code_bits=%d is not a container served: 8 (int8) or 4 (packed int4)", code_bits);
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

FQ_API int fqw_attn_cached_codes_workspace(int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t D, int64_t Smax, int64_t cus, int dtype, int code_bits,
                                           size_t* bytes, int64_t* nsplit) {
    const CccShape s{B, H, Hkv, T, D, Smax, cus};
    if (const int rc = ccc_shape(s, dtype, code_bits); rc != ROW_CONTINUE) return rc;
    if (!bytes || !nsplit) return fail(FQ_ERR_NULL, "bytes / nsplit must not be NULL");
    *nsplit = s.nsplit();
    *bytes = s.ws_bytes();
    return ok();
}

FQ_API int fqw_attn_cached_codes_fwd(const void* q, const void* k_codes_new, const float* k_t2_new, const void* v_codes_new, const float* v_t2_new,
                                     void* k_code_cache, float* k_t2_cache, void* v_code_cache, float* v_t2_cache, const int32_t* cache_lens,
                                     const int32_t* cache_starts, const void* cos, const void* sin, void* out, void* workspace, size_t workspace_bytes,
                                     int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t kn_sb, int64_t kn_sh, int64_t kn_st, int64_t vn_sb, int64_t vn_sh,
                                     int64_t vn_st, int64_t kc_sb, int64_t kc_sh, int64_t kc_st, int64_t vc_sb, int64_t vc_sh, int64_t vc_st, int64_t kt2n_bs,
                                     int64_t vt2n_bs, int64_t kt2c_bs, int64_t vt2c_bs, int64_t P, int64_t B, int64_t H, int64_t Hkv, int64_t T, int64_t Smax,
                                     int64_t D, int64_t cus, float inv, int dtype, int code_bits, void* stream) {
    const CccShape s{B, H, Hkv, T, D, Smax, cus};
    if (const int rc = ccc_shape(s, dtype, code_bits); rc != ROW_CONTINUE) return rc;
    const int64_t st[19] = {q_sb, q_sh, q_st, kn_sb, kn_sh, kn_st, vn_sb, vn_sh, vn_st, kc_sb, kc_sh, kc_st, vc_sb, vc_sh, vc_st, kt2n_bs, vt2n_bs, kt2c_bs, vt2c_bs};
    for (const int64_t x : st)
        if (x < 0) return fail(FQ_ERR_SHAPE, "negative stride %lld", (long long)x);
    if ((cos || sin) && (P <= 0 || P >= ((int64_t)1 << 50))) return fail(FQ_ERR_SHAPE, "P=%lld table rows must be positive", (long long)P);
    const int64_t cd = D * code_bits / 8;      // bytes of a key's codes
    auto t2_extent = [&](int64_t bs, int64_t n) {      // [B, n] fp32 by batch stride, in bytes
        const int64_t one[3] = {bs, 0, 0};
        return 4 * extent(B, one, 1, 1, n);
    };
    const int64_t nq = 2 * extent(B, st, H, T, D), nkn = extent(B, st + 3, Hkv, T, cd), nvn = extent(B, st + 6, Hkv, T, cd);
    const int64_t nkc = extent(B, st + 9, Hkv, Smax, cd), nvc = extent(B, st + 12, Hkv, Smax, cd);
    const int64_t nktn = t2_extent(kt2n_bs, T), nvtn = t2_extent(vt2n_bs, T), nktc = t2_extent(kt2c_bs, Smax), nvtc = t2_extent(vt2c_bs, Smax);
    if (!nq || !nkn || !nvn || !nkc || !nvc || !nktn || !nvtn || !nktc || !nvtc) return fail(FQ_ERR_SHAPE, "a tensor's extent overflows");
    if (!q || !k_codes_new || !k_t2_new || !v_codes_new || !v_t2_new || !k_code_cache || !k_t2_cache || !v_code_cache || !v_t2_cache || !cache_lens || !out)
        return fail(FQ_ERR_NULL, "q / the new codes and divisors / the four caches / cache_lens / out must not be NULL");
    if ((cos == nullptr) != (sin == nullptr)) return fail(FQ_ERR_NULL, "cos and sin come together or not at all");
    const Range reads[5] = {{q, nq}, {k_codes_new, nkn}, {v_codes_new, nvn}, {k_t2_new, nktn}, {v_t2_new, nvtn}};
    const Range caches[4] = {{k_code_cache, nkc}, {v_code_cache, nvc}, {k_t2_cache, nktc}, {v_t2_cache, nvtc}};
    for (const Range& r : reads)
        for (const Range& c : caches)
            if (overlap(r, c)) return fail(FQ_ERR_ARG, "q or a new tensor overlaps a cache: the append is in place and would race the reads");
    for (int i = 0; i < 4; ++i)
        for (int k = i + 1; k < 4; ++k)
            if (overlap(caches[i], caches[k])) return fail(FQ_ERR_ARG, "two caches overlap");
    const void* others[13] = {q, k_codes_new, k_t2_new, v_codes_new, v_t2_new, k_code_cache, k_t2_cache, v_code_cache, v_t2_cache, cache_lens, cache_starts, cos, sin};
    for (const void* p : others)
        if (p && (p == out || p == workspace)) return fail(FQ_ERR_ARG, "in-place (out or the workspace on another argument) is not supported");
    if (workspace && workspace == out) return fail(FQ_ERR_ARG, "in-place (the workspace on out) is not supported");
    const int64_t nsplit = s.nsplit();
    const size_t need = s.ws_bytes();
    if (need && (!workspace || workspace_bytes < need))
        return fail(FQ_ERR_UNSUPPORTED, "workspace too small: %zu bytes, fqw_attn_cached_codes_workspace asks for %zu", workspace ? workspace_bytes : (size_t)0, need);
    if (s.wgs() > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "B * Hkv * packs = %lld exceeds one launch's grid", (long long)s.wgs());

    CccArgs ca{};
    DecArgs& a = ca.d;
    a.q = q, a.out = out, a.ws = need ? (float*)workspace : nullptr, a.inv = inv;
    a.H = H, a.T = T, a.S = Smax, a.nsplit = (int)nsplit, a.Hkv = Hkv, a.G = s.G(), a.HP = s.HP(), a.NP = s.NP();
    ca.kn = (const uint8_t*)k_codes_new, ca.vn = (const uint8_t*)v_codes_new, ca.kc = (uint8_t*)k_code_cache, ca.vc = (uint8_t*)v_code_cache;
    for (int i = 0; i < 3; ++i) a.qs[i] = st[i], ca.kns[i] = st[3 + i], ca.vns[i] = st[6 + i], ca.kcs[i] = st[9 + i], ca.vcs[i] = st[12 + i];
    ca.kt2n = k_t2_new, ca.vt2n = v_t2_new, ca.kt2c = k_t2_cache, ca.vt2c = v_t2_cache;
    ca.kt2n_bs = kt2n_bs, ca.vt2n_bs = vt2n_bs, ca.kt2c_bs = kt2c_bs, ca.vt2c_bs = vt2c_bs;
    ca.cos = cos, ca.sin = sin, ca.P = P, ca.lens = cache_lens, ca.starts = cache_starts;
    const bool vec = aligned16(q) && aligned16(k_codes_new) && aligned16(v_codes_new) && aligned16(k_code_cache) && aligned16(v_code_cache) && mult(a.qs, 8) &&
                     mult(ca.kns, 16) && mult(ca.vns, 16) && mult(ca.kcs, 16) && mult(ca.vcs, 16) && (!cos || (aligned16(cos) && aligned16(sin)));
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    auto with = [&](auto sd, auto dd, auto cb, auto rot, auto vv) {
        constexpr int DT = decltype(sd)::value;
        launch_grid(ccc_kernel<DT, decltype(dd)::value, decltype(cb)::value, decltype(rot)::value != 0, decltype(vv)::value != 0>, s.wgs(), nsplit,
                    DEC_WAVES * 64, stm, ca);
        if (nsplit > 1)
            launch_grid(gqa_combine_kernel<DT>, s.wgs(), a.HP * a.T, (int)D, stm, (const float*)a.ws, out, H, a.G, a.HP, a.NP, T, (int)D, (int)nsplit);
    };
    auto by_dt = [&](auto sd) {
        auto by_d = [&](auto dd) {
            auto by_cb = [&](auto cb) {
                auto by_rot = [&](auto rot) { vec ? with(sd, dd, cb, rot, Const<1>{}) : with(sd, dd, cb, rot, Const<0>{}); };
                cos ? by_rot(Const<1>{}) : by_rot(Const<0>{});
            };
            code_bits == 8 ? by_cb(Const<8>{}) : by_cb(Const<4>{});
        };
        D == 64 ? by_d(Const<64>{}) : by_d(Const<128>{});
    };
    if (dtype == FQ_DTYPE_BF16) by_dt(Const<BF16>{});
    else by_dt(Const<F16>{});
    return launch_result();
}

}  // extern "C"
