// fq_attn_train.hip -- the training attention (include/llmqat_fakequant_attn_train.h): the forward kernel of fq_attn_prefill.h with its
// statistics output, the two backward kernels of fq_attn_train.h, and their entry points: a translation unit of its own, so the other
// units compile exactly as before.
#include "../../include/llmqat_fakequant_attn_train.h"

#include "fq_attn_train.h"

using namespace fq;

namespace {

// the largest element offset of a [n0, n1, n2, D] view by strides fits 62 bits
bool span_ok(int64_t n0, int64_t s0, int64_t n1, int64_t s1, int64_t n2, int64_t s2, int64_t D) {
    const __int128 top = (__int128)(n0 - 1) * s0 + (__int128)(n1 - 1) * s1 + (__int128)(n2 - 1) * s2 + D;
    return top < ((__int128)1 << 62);
}

bool strides_vec(const int64_t* st) { return st[0] % 8 == 0 && st[1] % 8 == 0 && st[2] % 8 == 0; }

// the refusals both entry points share, in the header's order up to FQ_ERR_SHAPE; st: nv views of three strides each (q, k, v first)
int check_dtype_shape(const int64_t* st, int nv, const void* mask, int64_t mbs, int64_t mrs, int64_t B, int64_t H, int64_t T, int64_t S,
                      int64_t D, int dtype, int mask_dtype, int causal, const char* who) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16)
        return fail(FQ_ERR_DTYPE, "dtype code %d is not served by the training attention's %s: bfloat16 or float16 q, k, v", dtype, who);
    if (mask && (mask_dtype < 0 || mask_dtype > FQ_DTYPE_F64)) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", mask_dtype);
    if (mask && mask_dtype != dtype && mask_dtype != FQ_DTYPE_F32)
        return fail(FQ_ERR_DTYPE, "the dtype pair (q, k, v %d, mask %d) is not served: a mask in their dtype or in float32", dtype, mask_dtype);
    if (B <= 0 || H <= 0 || T <= 0 || S <= 0)
        return fail(FQ_ERR_SHAPE, "B=%lld H=%lld T=%lld S=%lld must be positive", (long long)B, (long long)H, (long long)T, (long long)S);
    if (D != 64 && D != 128) return fail(FQ_ERR_SHAPE, "D=%lld is not a head size served (64, 128)", (long long)D);
    for (int i = 0; i < 3 * nv; ++i)
        if (st[i] < 0) return fail(FQ_ERR_SHAPE, "negative stride %lld", (long long)st[i]);
    if (mask && (mbs < 0 || mrs < 0)) return fail(FQ_ERR_SHAPE, "negative mask stride (batch %lld, row %lld)", (long long)mbs, (long long)mrs);
    if (B > INT64_MAX / H || (__int128)(B * H) * T * D >= ((__int128)1 << 62) || (__int128)(B * H) * S * D >= ((__int128)1 << 62))
        return fail(FQ_ERR_SHAPE, "B * H * T * D or B * H * S * D overflows");
    for (int i = 0; i < nv; ++i)
        if (!span_ok(B, st[3 * i], H, st[3 * i + 1], i == 1 || i == 2 ? S : T, st[3 * i + 2], D)) return fail(FQ_ERR_SHAPE, "a tensor's extent overflows");
    if (mask && !span_ok(B, mbs, T, mrs, 1, 0, S)) return fail(FQ_ERR_SHAPE, "a tensor's extent overflows");
    if (causal && T > S) return fail(FQ_ERR_SHAPE, "causal: T=%lld query rows are the last of S=%lld keys, so T <= S", (long long)T, (long long)S);
    return 0;
}

struct MaskKind {
    int kind;       // 0: none, 1: the tensors' dtype, 2: float32, 3: causal
    bool vec;       // the mask's vector loads
};
MaskKind mask_kind(const void* mask, int64_t mbs, int64_t mrs, int dtype, int mask_dtype, int causal) {
    const int kind = causal ? 3 : !mask ? 0 : mask_dtype == dtype ? 1 : 2;
    const uintptr_t align = kind == 2 ? 15u : 7u;
    return {kind, mask && (reinterpret_cast<uintptr_t>(mask) & align) == 0 && mbs % 4 == 0 && mrs % 4 == 0};
}

// f(dtype, mask dtype, causal, D, vec, mvec) as Const<> values
template <class F> void dispatch(int dtype, MaskKind mk, int64_t D, bool vec, F&& f) {
    auto by_dt = [&](auto sd) {
        constexpr int DT = decltype(sd)::value;
        auto by_d = [&](auto md, auto cz, auto mv) {
            if (D == 64) vec ? f(sd, md, cz, Const<64>{}, Const<1>{}, mv) : f(sd, md, cz, Const<64>{}, Const<0>{}, mv);
            else vec ? f(sd, md, cz, Const<128>{}, Const<1>{}, mv) : f(sd, md, cz, Const<128>{}, Const<0>{}, mv);
        };
        if (mk.kind == 0) by_d(Const<ATTN_NOMASK>{}, Const<0>{}, Const<0>{});
        else if (mk.kind == 3) by_d(Const<ATTN_NOMASK>{}, Const<1>{}, Const<0>{});
        else if (mk.kind == 1) mk.vec ? by_d(Const<DT>{}, Const<0>{}, Const<1>{}) : by_d(Const<DT>{}, Const<0>{}, Const<0>{});
        else mk.vec ? by_d(Const<F32>{}, Const<0>{}, Const<1>{}) : by_d(Const<F32>{}, Const<0>{}, Const<0>{});
    };
    if (dtype == FQ_DTYPE_BF16) by_dt(Const<BF16>{});
    else by_dt(Const<F16>{});
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqg_attn_train_fwd(const void* q, const void* k, const void* v, const void* mask, void* out, float* stats, int64_t q_sb, int64_t q_sh,
                              int64_t q_st, int64_t k_sb, int64_t k_sh, int64_t k_st, int64_t v_sb, int64_t v_sh, int64_t v_st,
                              int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H, int64_t T, int64_t S, int64_t D,
                              float inv, int dtype, int mask_dtype, int causal, void* stream) {
    const int64_t st[9] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st};
    if (const int rc = check_dtype_shape(st, 3, mask, mask_batch_stride, mask_row_stride, B, H, T, S, D, dtype, mask_dtype, causal, "forward")) return rc;
    if (!q || !k || !v || !out) return fail(FQ_ERR_NULL, "q / k / v / out must not be NULL");
    const void* ins[4] = {q, k, v, mask};
    for (const void* p : ins)
        if (p && (p == out || p == stats)) return fail(FQ_ERR_ARG, "in-place (out or stats on an input) is not supported");
    if (out == stats) return fail(FQ_ERR_ARG, "out and stats are one pointer");
    if (causal && mask) return fail(FQ_ERR_ARG, "causal together with a mask: give one of them");
    const int64_t nqt = pre_query_tiles(T);
    if (B * H > PRE_MAX_GRID_Y || nqt > 0x7FFFFFFF)
        return fail(FQ_ERR_UNSUPPORTED, "B * H = %lld or %lld query tiles exceed one launch's grid", (long long)(B * H), (long long)nqt);

    PreArgs a{};
    a.q = q, a.k = k, a.v = v, a.mask = mask, a.out = out, a.stats = stats;
    for (int i = 0; i < 3; ++i) a.qs[i] = st[i], a.ks[i] = st[3 + i], a.vs[i] = st[6 + i];
    a.mbs = mask ? mask_batch_stride : 0, a.mrs = mask ? mask_row_stride : 0;
    a.H = H, a.T = T, a.S = S, a.inv = inv;
    const bool vec = aligned16(q) && aligned16(k) && aligned16(v) && strides_vec(a.qs) && strides_vec(a.ks) && strides_vec(a.vs);
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    dispatch(dtype, mask_kind(mask, a.mbs, a.mrs, dtype, mask_dtype, causal), D, vec, [&](auto sd, auto md, auto cz, auto dd, auto vv, auto mv) {
        launch_grid(pre_kernel<decltype(sd)::value, decltype(md)::value, decltype(cz)::value != 0, decltype(dd)::value, PRE_RPW / 16,
                               decltype(vv)::value != 0, decltype(mv)::value != 0, true>,
                    nqt, B * H, PRE_WAVES * 64, stm, a);
    });
    return launch_result();
}

FQ_API int fqg_attn_train_bwd(const void* q, const void* k, const void* v, const void* mask, const void* out, const void* dout, const float* stats,
                              float* delta, void* dq, void* dk, void* dv, int64_t q_sb, int64_t q_sh, int64_t q_st, int64_t k_sb, int64_t k_sh,
                              int64_t k_st, int64_t v_sb, int64_t v_sh, int64_t v_st, int64_t o_sb, int64_t o_sh, int64_t o_st, int64_t g_sb,
                              int64_t g_sh, int64_t g_st, int64_t mask_batch_stride, int64_t mask_row_stride, int64_t B, int64_t H, int64_t T,
                              int64_t S, int64_t D, float inv, int dtype, int mask_dtype, int causal, void* stream) {
    const int64_t st[15] = {q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st, g_sb, g_sh, g_st};
    if (const int rc = check_dtype_shape(st, 5, mask, mask_batch_stride, mask_row_stride, B, H, T, S, D, dtype, mask_dtype, causal, "backward")) return rc;
    if (!q || !k || !v || !out || !dout || !stats || !delta || !dq || !dk || !dv)
        return fail(FQ_ERR_NULL, "q / k / v / out / dout / stats / delta / dq / dk / dv must not be NULL");
    const void* ins[7] = {q, k, v, mask, out, dout, stats};
    const void* outs[4] = {delta, dq, dk, dv};
    for (int i = 0; i < 4; ++i) {
        for (const void* p : ins)
            if (p && p == outs[i]) return fail(FQ_ERR_ARG, "in-place (delta, dq, dk or dv on an input) is not supported");
        for (int n = 0; n < i; ++n)
            if (outs[n] == outs[i]) return fail(FQ_ERR_ARG, "delta, dq, dk and dv are four buffers: two of them are one pointer");
    }
    if (causal && mask) return fail(FQ_ERR_ARG, "causal together with a mask: give one of them");
    const int64_t nqt = trn_query_tiles(T), nkt = trn_key_tiles(S);
    if (B * H > PRE_MAX_GRID_Y || nqt > 0x7FFFFFFF || nkt > 0x7FFFFFFF)
        return fail(FQ_ERR_UNSUPPORTED, "B * H = %lld, %lld query tiles or %lld key tiles exceed one launch's grid", (long long)(B * H),
                    (long long)nqt, (long long)nkt);

    TrnArgs a{};
    a.q = q, a.k = k, a.v = v, a.mask = mask, a.out = out, a.dout = dout, a.stats = stats, a.delta = delta, a.dq = dq, a.dk = dk, a.dv = dv;
    for (int i = 0; i < 3; ++i) a.qs[i] = st[i], a.ks[i] = st[3 + i], a.vs[i] = st[6 + i], a.os[i] = st[9 + i], a.gs[i] = st[12 + i];
    a.mbs = mask ? mask_batch_stride : 0, a.mrs = mask ? mask_row_stride : 0;
    a.H = H, a.T = T, a.S = S, a.inv = inv;
    const bool vec = aligned16(q) && aligned16(k) && aligned16(v) && aligned16(out) && aligned16(dout) && strides_vec(a.qs) &&
                     strides_vec(a.ks) && strides_vec(a.vs) && strides_vec(a.os) && strides_vec(a.gs);
    const MaskKind mk = mask_kind(mask, a.mbs, a.mrs, dtype, mask_dtype, causal);
    hipStream_t stm = (hipStream_t)stream;
    begin_launches();
    dispatch(dtype, mk, D, vec, [&](auto sd, auto md, auto cz, auto dd, auto vv, auto mv) {
        launch_grid(trn_dq_kernel<decltype(sd)::value, decltype(md)::value, decltype(cz)::value != 0, decltype(dd)::value, TRN_RPW / 16,
                                  decltype(vv)::value != 0, decltype(mv)::value != 0>,
                    nqt, B * H, TRN_WAVES * 64, stm, a);
    });
    dispatch(dtype, MaskKind{mk.kind, false}, D, vec, [&](auto sd, auto md, auto cz, auto dd, auto vv, auto) {      // element loads of the mask
        launch_grid(trn_dkv_kernel<decltype(sd)::value, decltype(md)::value, decltype(cz)::value != 0, decltype(dd)::value, TRN_KPW / 16,
                                   decltype(vv)::value != 0>,
                    nkt, B * H, TRN_WAVES * 64, stm, a);
    });
    return launch_result();
}

}  // extern "C"
