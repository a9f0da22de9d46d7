// fq_attn_softmax.hip -- the attention-softmax kernels (fq_attn_softmax.h) and their entry points (include/llmqat_fakequant_attn.h): a
// translation unit of its own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_attn.h"

#include "fq_attn_softmax.h"

using namespace fq;

namespace {

struct AttnShape {
    int64_t rows, cols, B, H, T, mbs, mrs;
};

// what both entry points check first, in the header's order: ROW_CONTINUE, or the refusal.  Every check comes before any HIP call.
int attn_head(const AttnShape& s, const void* mask, int s_dtype, int m_dtype) {
    const int rc = mask ? row_head("attention softmax", s.rows, s.cols, {s_dtype, m_dtype}, [&] {
        if (m_dtype == s_dtype || m_dtype == FQ_DTYPE_F32) return ROW_CONTINUE;
        return fail(FQ_ERR_DTYPE, "the dtype pair (scores %d, mask %d) is not served: a mask in the scores' dtype or in float32", s_dtype, m_dtype);
    }) : row_head("attention softmax", s.rows, s.cols, {s_dtype});
    if (rc != ROW_CONTINUE) return rc;
    if (s.B <= 0 || s.H <= 0 || s.T <= 0) return fail(FQ_ERR_SHAPE, "B=%lld H=%lld T=%lld must be positive", (long long)s.B, (long long)s.H, (long long)s.T);
    if (s.rows % s.T) return fail(FQ_ERR_SHAPE, "rows=%lld is not a multiple of T=%lld", (long long)s.rows, (long long)s.T);
    if ((s.rows / s.T) % s.H || s.rows / s.T / s.H != s.B)
        return fail(FQ_ERR_SHAPE, "rows=%lld is not B * H * T = %lld * %lld * %lld", (long long)s.rows, (long long)s.B, (long long)s.H, (long long)s.T);
    if (mask && (s.mbs < 0 || s.mrs < 0)) return fail(FQ_ERR_SHAPE, "negative mask stride (batch %lld, row %lld)", (long long)s.mbs, (long long)s.mrs);
    return ROW_CONTINUE;
}

AttnMask attn_mask(const AttnShape& s, const void* mask) { return AttnMask{mask, s.mbs, s.mrs, s.H * s.T, s.T}; }

// 16-byte accesses: the row layer's condition on the scores-shaped tensors, and every mask row on a 16-byte boundary
bool attn_vec(const AttnShape& s, int s_dtype, int m_dtype, const void* mask, const void* p0, const void* p1, const void* p2 = nullptr, const void* p3 = nullptr) {
    if (!row_vec(s.cols, s_dtype, p0, p1, p2) || !aligned16(p3)) return false;
    const int64_t me = esize_of(m_dtype);
    return !mask || (aligned16(mask) && s.mbs * me % 16 == 0 && s.mrs * me % 16 == 0);
}

// the kernel <DT, MDT, VEC, TPR, NGV> of a served call: f(Const<DT>, Const<MDT>, Const<VEC>, Const<TPR>, Const<NGV>).  MDT: the scores'
// dtype, F32, or ATTN_NOMASK.  The 16-byte kernels are built for 8, 16 and 32 slots of a lane: the smallest that holds the row (a
// function of cols alone, so the summation order is one too); the element path has one form (NGV = 0)
template <class F> int by_attn_kernel(int s_dtype, int m_kind /* 0 none, 1 same, 2 f32 */, int64_t cols, bool vec, F&& f) {
    return by_dtype(s_dtype, [&](auto sd) {
        constexpr int DT = decltype(sd)::value;
        auto shape = [&](auto md) {
            constexpr int MDT = decltype(md)::value;
            by_row_shape(cols, vec, [&](auto v, auto tpr) {
                constexpr int V = decltype(v)::value, TPR = decltype(tpr)::value;
                if constexpr (V == 0) {
                    f(Const<DT>{}, Const<MDT>{}, Const<0>{}, Const<TPR>{}, Const<0>{});
                } else {
                    constexpr int MOST = attn_most_groups<DT>();
                    const int64_t need = (cols * Ty<DT>::ESIZE / 16 + TPR - 1) / TPR;      // vectors of a lane
                    if (need <= attn_groups(MOST, 2)) f(Const<DT>{}, Const<MDT>{}, Const<1>{}, Const<TPR>{}, Const<attn_groups(MOST, 2)>{});
                    else if (need <= attn_groups(MOST, 1)) f(Const<DT>{}, Const<MDT>{}, Const<1>{}, Const<TPR>{}, Const<attn_groups(MOST, 1)>{});
                    else f(Const<DT>{}, Const<MDT>{}, Const<1>{}, Const<TPR>{}, Const<MOST>{});
                }
            });
        };
        if (m_kind == 0) shape(Const<ATTN_NOMASK>{});
        else if (m_kind == 1 || DT == F32) shape(Const<DT>{});
        else shape(Const<F32>{});
        return launch_result();
    });
}

int mask_kind(const void* mask, int s_dtype, int m_dtype) { return !mask ? 0 : m_dtype == s_dtype ? 1 : 2; }

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqs2_attn_softmax_fwd(const void* scores, const void* mask, void* y, float* stats, int64_t rows, int64_t cols, int64_t B, int64_t H,
                                 int64_t T, int64_t mask_batch_stride, int64_t mask_row_stride, float inv, int scores_dtype, int mask_dtype,
                                 void* stream) {
    const AttnShape s{rows, cols, B, H, T, mask_batch_stride, mask_row_stride};
    if (const int rc = attn_head(s, mask, scores_dtype, mask_dtype); rc != ROW_CONTINUE) return rc;
    if (!scores || !y) return fail(FQ_ERR_NULL, "scores / y must not be NULL");
    if (y == scores || y == mask || (stats && ((const void*)stats == scores || (const void*)stats == mask || (void*)stats == y)))
        return fail(FQ_ERR_ARG, "in-place (y or stats on an input, stats on y) is not supported");
    if (const int rc = row_grid_check(rows, cols); rc != ROW_CONTINUE) return rc;
    const AttnFwdArgs a{scores, attn_mask(s, mask), y, stats, rows, cols, inv};
    const bool vec = attn_vec(s, scores_dtype, mask_dtype, mask, scores, y);
    hipStream_t st = (hipStream_t)stream;
    begin_launches();
    return by_attn_kernel(scores_dtype, mask_kind(mask, scores_dtype, mask_dtype), cols, vec, [&](auto sd, auto md, auto v, auto tpr, auto ng) {
        launch_rows<decltype(tpr)::value>(attn_fwd_kernel<decltype(sd)::value, decltype(md)::value, decltype(v)::value != 0, decltype(tpr)::value, decltype(ng)::value>,
                                          rows, st, a);
    });
}

FQ_API int fqs2_attn_softmax_bwd(const void* g, const void* scores, const void* mask, const float* stats, void* dx, int64_t rows, int64_t cols,
                                 int64_t B, int64_t H, int64_t T, int64_t mask_batch_stride, int64_t mask_row_stride, float inv, int scores_dtype,
                                 int mask_dtype, void* stream) {
    const AttnShape s{rows, cols, B, H, T, mask_batch_stride, mask_row_stride};
    if (const int rc = attn_head(s, mask, scores_dtype, mask_dtype); rc != ROW_CONTINUE) return rc;
    if (!g || !scores || !stats || !dx) return fail(FQ_ERR_NULL, "g / scores / stats / dx must not be NULL");
    if (dx == g || dx == scores || dx == mask || dx == (const void*)stats) return fail(FQ_ERR_ARG, "in-place (dx == g, scores, mask or stats) is not supported");
    if (const int rc = row_grid_check(rows, cols); rc != ROW_CONTINUE) return rc;
    const AttnBwdArgs a{g, scores, attn_mask(s, mask), stats, dx, rows, cols, inv};
    const bool vec = attn_vec(s, scores_dtype, mask_dtype, mask, g, scores, dx);
    hipStream_t st = (hipStream_t)stream;
    begin_launches();
    return by_attn_kernel(scores_dtype, mask_kind(mask, scores_dtype, mask_dtype), cols, vec, [&](auto sd, auto md, auto v, auto tpr, auto ng) {
        launch_rows<decltype(tpr)::value>(attn_bwd_kernel<decltype(sd)::value, decltype(md)::value, decltype(v)::value != 0, decltype(tpr)::value, decltype(ng)::value>,
                                          rows, st, a);
    });
}

}  // extern "C"
