// fq_rope.hip -- the rotary embedding kernels (fq_rope.h) and their entry points (include/llmqat_fakequant_rope.h): a translation unit
// of its own, entry points included, so the other units compile exactly as before.
#include "../../include/llmqat_fakequant_rope.h"

#include "fq_rope.h"

using namespace fq;

namespace {

constexpr int64_t MOST = INT64_MAX / 4;

struct RopeShape {
    int64_t B, Hq, Hk, T, D, P;
};

// the strides of the dense output of an input [B, H, T, D] with strides s: the header's rule.  An insertion sort from the innermost
// place outwards, as ATen's elementwise ops order their dimensions; a dimension of size 1 or of stride 0 compares equal to every other
void dense_strides(const int64_t (&n)[3], int64_t D, const int64_t (&s)[3], int64_t (&out)[3]) {
    int perm[3] = {2, 1, 0};                                   // innermost first
    auto cmp = [&](int d0, int d1) {
        if (n[d0] == 1 || n[d1] == 1 || s[d0] == 0 || s[d1] == 0) return 0;
        if (s[d0] != s[d1]) return s[d0] < s[d1] ? -1 : 1;
        return n[d0] > n[d1] ? 1 : 0;
    };
    for (int i = 1; i < 3; ++i) {
        int d1 = i;
        for (int d0 = i - 1; d0 >= 0; --d0) {
            const int c = cmp(perm[d0], perm[d1]);
            if (c > 0) {
                std::swap(perm[d0], perm[d1]);
                d1 = d0;
            } else if (c < 0) {
                break;
            }
        }
    }
    int64_t acc = D;
    for (const int d : perm) {
        out[d] = acc;
        acc *= n[d];
    }
}

// what both entry points check first, in the header's order: ROW_CONTINUE, or the refusal.  Every check comes before any HIP call.
// strides: (batch, head, token) triples, each with the heads of its tensor
struct Strided {
    const char* name;
    int64_t H;
    const int64_t (&s)[3];
};
int rope_head(const RopeShape& z, int q_dtype, int k_dtype, int table_dtype, int64_t pos_bs, std::initializer_list<Strided> tensors) {
    for (const int dt : {q_dtype, k_dtype, table_dtype}) {
        if (dt < 0 || dt > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dt);
        if (dt == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the rotary embedding entry points");
    }
    if (q_dtype != k_dtype && q_dtype != FQ_DTYPE_F32 && k_dtype != FQ_DTYPE_F32)
        return fail(FQ_ERR_DTYPE, "q and k in two dtypes: one of them is float32 (q_dtype=%d k_dtype=%d)", q_dtype, k_dtype);
    if (q_dtype != k_dtype && table_dtype != FQ_DTYPE_F32)
        return fail(FQ_ERR_DTYPE, "q and k in two dtypes take float32 tables: table_dtype=%d", table_dtype);
    if (table_dtype != q_dtype && table_dtype != FQ_DTYPE_F32)
        return fail(FQ_ERR_DTYPE, "the tables are in the tensors' dtype or in float32: dtype=%d table_dtype=%d", q_dtype, table_dtype);
    if (z.B <= 0 || z.Hq <= 0 || z.Hk <= 0 || z.T <= 0 || z.D <= 0)
        return fail(FQ_ERR_SHAPE, "non-positive shape B=%lld Hq=%lld Hk=%lld T=%lld D=%lld", (long long)z.B, (long long)z.Hq, (long long)z.Hk,
                    (long long)z.T, (long long)z.D);
    if (z.D % 2) return fail(FQ_ERR_SHAPE, "odd head size D=%lld: a rotation pairs the two halves of a head", (long long)z.D);
    if (z.P <= 0) return fail(FQ_ERR_SHAPE, "non-positive table rows P=%lld", (long long)z.P);
    if (z.P > MOST / z.D) return fail(FQ_ERR_SHAPE, "P * D overflows");
    if (pos_bs != 0 && pos_bs != z.T) return fail(FQ_ERR_SHAPE, "pos_batch_stride=%lld is neither 0 nor T=%lld", (long long)pos_bs, (long long)z.T);
    for (const Strided& t : tensors) {
        const int64_t n[3] = {z.B, t.H, z.T};
        int64_t count = z.D, extent = z.D;
        for (int d = 0; d < 3; ++d) {
            if (t.s[d] < 0) return fail(FQ_ERR_SHAPE, "negative stride %lld of %s", (long long)t.s[d], t.name);
            if (n[d] > MOST / count) return fail(FQ_ERR_SHAPE, "the element count of %s overflows", t.name);
            count *= n[d];
            if (n[d] > 1 && t.s[d] > (MOST - extent) / (n[d] - 1)) return fail(FQ_ERR_SHAPE, "the extent of %s overflows", t.name);
            extent += (n[d] - 1) * t.s[d];
        }
    }
    return ROW_CONTINUE;
}

int rope_grid_check(const RopeShape& z) {
    if (z.B > 0x7FFFFFFF / z.T) return fail(FQ_ERR_UNSUPPORTED, "B * T = %lld * %lld tokens exceed one launch's grid", (long long)z.B, (long long)z.T);
    if (z.Hq + z.Hk > (int64_t(1) << 30) / (z.D / 2))
        return fail(FQ_ERR_UNSUPPORTED, "(Hq + Hk) * D / 2 exceeds 2^30: Hq=%lld Hk=%lld D=%lld", (long long)z.Hq, (long long)z.Hk, (long long)z.D);
    return ROW_CONTINUE;
}

bool strides_vec(const RopeSide& s, int64_t xes, int64_t yes) {
    if (!s.H) return true;
    bool v = aligned16(s.x) && aligned16(s.y);
    for (int d = 0; d < 3; ++d) v = v && s.xs[d] * xes % 16 == 0 && s.ys[d] * yes % 16 == 0;
    return v;
}

// q and k in two dtypes (rope_mixed_kernel): the 16-bit side reads (forward) or writes (backward) 2-byte elements, everything else is fp32
template <bool BWD> int rope_launch_mixed(RopeArgs& a, const RopeShape& z, int q_dtype, int k_dtype, hipStream_t st) {
    a.s[0].narrow = q_dtype != FQ_DTYPE_F32;
    a.s[1].narrow = k_dtype != FQ_DTYPE_F32;
    bool vec = a.h % 8 == 0 && aligned16(a.cos) && aligned16(a.sin);
    for (const RopeSide& s : a.s) vec = vec && strides_vec(s, !BWD && s.narrow ? 2 : 4, BWD && s.narrow ? 2 : 4);
    const dim3 grid((unsigned)(z.B * z.T));
    return by_dtype(a.s[0].narrow ? q_dtype : k_dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if constexpr (DT == F32) {
            return fail(FQ_ERR_DTYPE, "q and k in two dtypes: one of them is 16-bit");      // (not reached: rope_head has refused it)
        } else {
            begin_launches();
            if (vec) launch(rope_mixed_kernel<DT, true, BWD>, grid, dim3(ROW_TPB), st, a);
            else launch(rope_mixed_kernel<DT, false, BWD>, grid, dim3(ROW_TPB), st, a);
            return launch_result();
        }
    });
}

template <bool BWD> int rope_launch(RopeArgs& a, const RopeShape& z, int dtype, int k_dtype, int table_dtype, hipStream_t st) {
    if (dtype != k_dtype) return rope_launch_mixed<BWD>(a, z, dtype, k_dtype, st);
    const int64_t es = esize_of(dtype);
    const bool vec = a.h * es % 16 == 0 && aligned16(a.cos) && aligned16(a.sin) && strides_vec(a.s[0], es, es) && strides_vec(a.s[1], es, es);
    const bool tf32 = table_dtype == FQ_DTYPE_F32 && dtype != FQ_DTYPE_F32;
    const dim3 grid((unsigned)(z.B * z.T));
    return by_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        begin_launches();
        if constexpr (DT == F32) {
            if (vec) launch(rope_kernel<DT, true, false, BWD>, grid, dim3(ROW_TPB), st, a);
            else launch(rope_kernel<DT, false, false, BWD>, grid, dim3(ROW_TPB), st, a);
        } else {
            if (vec && tf32) launch(rope_kernel<DT, true, true, BWD>, grid, dim3(ROW_TPB), st, a);
            else if (vec) launch(rope_kernel<DT, true, false, BWD>, grid, dim3(ROW_TPB), st, a);
            else if (tf32) launch(rope_kernel<DT, false, true, BWD>, grid, dim3(ROW_TPB), st, a);
            else launch(rope_kernel<DT, false, false, BWD>, grid, dim3(ROW_TPB), st, a);
        }
        return launch_result();
    });
}

// live = false: the side has no items in this launch (H = 0 in the kernel's eyes)
void fill_side(RopeSide& s, bool live, const void* x, void* y, int64_t B, int64_t H, int64_t T, int64_t D, const int64_t (&xs)[3],
               const int64_t (&order)[3]) {
    s.x = x;
    s.y = y;
    s.H = live ? (int32_t)H : 0;
    s.narrow = 0;
    const int64_t n[3] = {B, H, T};
    for (int d = 0; d < 3; ++d) s.xs[d] = xs[d];
    dense_strides(n, D, order, s.ys);
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fqr_rope_dense_strides(int64_t B, int64_t H, int64_t T, int64_t D, int64_t stride_b, int64_t stride_h, int64_t stride_t, int64_t* out) {
    if (B <= 0 || H <= 0 || T <= 0 || D <= 0)
        return fail(FQ_ERR_SHAPE, "non-positive shape B=%lld H=%lld T=%lld D=%lld", (long long)B, (long long)H, (long long)T, (long long)D);
    if (!out) return fail(FQ_ERR_NULL, "out must not be NULL");
    const int64_t n[3] = {B, H, T}, s[3] = {stride_b, stride_h, stride_t};
    int64_t o[3];
    dense_strides(n, D, s, o);
    for (int d = 0; d < 3; ++d) out[d] = o[d];
    return ok();
}

FQ_API int fqr_rope_fwd(const void* q, const void* k, void* q_out, void* k_out, const void* cos, const void* sin, const int64_t* positions,
                        int64_t pos_batch_stride, int64_t B, int64_t Hq, int64_t Hk, int64_t T, int64_t D, int64_t P, int64_t q_stride_b,
                        int64_t q_stride_h, int64_t q_stride_t, int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t, int q_dtype,
                        int k_dtype, int table_dtype, void* stream) {
    const RopeShape z{B, Hq, Hk, T, D, P};
    const int64_t qs[3] = {q_stride_b, q_stride_h, q_stride_t}, ks[3] = {k_stride_b, k_stride_h, k_stride_t};
    if (const int rc = rope_head(z, q_dtype, k_dtype, table_dtype, pos_batch_stride, {{"q", Hq, qs}, {"k", Hk, ks}}); rc != ROW_CONTINUE) return rc;
    if (!q || !k || !q_out || !k_out || !cos || !sin) return fail(FQ_ERR_NULL, "q / k / q_out / k_out / cos / sin must not be NULL");
    for (const void* o : {(const void*)q_out, (const void*)k_out})
        if (o == q || o == k || o == cos || o == sin) return fail(FQ_ERR_ARG, "in-place (an output that is q, k, cos or sin) is not supported");
    if (q_out == k_out) return fail(FQ_ERR_ARG, "q_out and k_out must not be the same buffer");
    if (const int rc = rope_grid_check(z); rc != ROW_CONTINUE) return rc;
    RopeArgs a{};
    fill_side(a.s[0], true, q, q_out, B, Hq, T, D, qs, qs);
    fill_side(a.s[1], true, k, k_out, B, Hk, T, D, ks, ks);
    a.cos = cos, a.sin = sin, a.pos = positions, a.pos_bs = pos_batch_stride, a.P = P, a.T = T, a.h = (int32_t)(D / 2);
    return rope_launch<false>(a, z, q_dtype, k_dtype, table_dtype, (hipStream_t)stream);
}

FQ_API int fqr_rope_bwd(const void* dq_out, const void* dk_out, void* dq, void* dk, const void* cos, const void* sin, const int64_t* positions,
                        int64_t pos_batch_stride, int64_t B, int64_t Hq, int64_t Hk, int64_t T, int64_t D, int64_t P, int64_t gq_stride_b,
                        int64_t gq_stride_h, int64_t gq_stride_t, int64_t gk_stride_b, int64_t gk_stride_h, int64_t gk_stride_t,
                        int64_t q_stride_b, int64_t q_stride_h, int64_t q_stride_t, int64_t k_stride_b, int64_t k_stride_h, int64_t k_stride_t,
                        int q_dtype, int k_dtype, int table_dtype, void* stream) {
    const RopeShape z{B, Hq, Hk, T, D, P};
    const int64_t gqs[3] = {gq_stride_b, gq_stride_h, gq_stride_t}, gks[3] = {gk_stride_b, gk_stride_h, gk_stride_t};
    const int64_t qs[3] = {q_stride_b, q_stride_h, q_stride_t}, ks[3] = {k_stride_b, k_stride_h, k_stride_t};
    if (const int rc = rope_head(z, q_dtype, k_dtype, table_dtype, pos_batch_stride, {{"dq_out", Hq, gqs}, {"dk_out", Hk, gks}, {"q", Hq, qs}, {"k", Hk, ks}});
        rc != ROW_CONTINUE)
        return rc;
    if (!cos || !sin) return fail(FQ_ERR_NULL, "cos / sin must not be NULL");
    if (!dq && !dk) return fail(FQ_ERR_NULL, "dq and dk must not both be NULL");
    if ((dq && !dq_out) || (dk && !dk_out)) return fail(FQ_ERR_NULL, "the incoming gradient of a side that is asked for must not be NULL");
    for (const void* o : {(const void*)dq, (const void*)dk})
        if (o && ((dq && o == dq_out) || (dk && o == dk_out) || o == cos || o == sin))
            return fail(FQ_ERR_ARG, "in-place (an output that is dq_out, dk_out, cos or sin) is not supported");
    if (dq == dk) return fail(FQ_ERR_ARG, "dq and dk must not be the same buffer");
    if (const int rc = rope_grid_check(z); rc != ROW_CONTINUE) return rc;
    RopeArgs a{};
    fill_side(a.s[0], dq != nullptr, dq_out, dq, B, Hq, T, D, gqs, qs);
    fill_side(a.s[1], dk != nullptr, dk_out, dk, B, Hk, T, D, gks, ks);
    a.cos = cos, a.sin = sin, a.pos = positions, a.pos_bs = pos_batch_stride, a.P = P, a.T = T, a.h = (int32_t)(D / 2);
    return rope_launch<true>(a, z, q_dtype, k_dtype, table_dtype, (hipStream_t)stream);
}

}  // extern "C"
