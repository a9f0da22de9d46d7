// fq_api.hip -- host side of the C ABI declared in include/llmqat_fakequant.h:
// argument validation, kernel selection, launches.  No allocation, no synchronisation.
#include "../../include/llmqat_fakequant.h"
#include "../../include/llmqat_fakequant_train.h"
#include "../../include/llmqat_fakequant_sr.h"
#include "../../include/llmqat_fakequant_infer.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "fq_launch.h"

using namespace fq;

namespace {
thread_local char g_err[320] = "";
}

namespace fq {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
int ok() {
    g_err[0] = 0;
    return FQ_OK;
}
hipError_t& launch_status() {
    static thread_local hipError_t st = hipSuccess;
    return st;
}
}  // namespace fq

namespace {

struct MaskArgs {
    void* mask;
    size_t bytes;
    float lo, hi;
};

// fq_rows_view (elements) -> RowPitch (bytes).  A view that describes contiguous rows stays off.  false: not representable.
bool set_pitch(RowPitch& p, const fq_rows_view* v, int64_t rows, int64_t cols, int esize) {
    p = RowPitch{};
    if (!v || v->n_inner <= 0) return true;
    if (rows > 0x7FFFFFFF || v->n_inner > 0x7FFFFFFF || v->stride_outer < 0 || v->stride_inner < 0) return false;
    if (v->stride_inner == cols && (v->n_inner >= rows || v->stride_outer == v->n_inner * cols)) return true;   // contiguous after all
    p.outer = v->stride_outer * esize;
    p.inner = v->stride_inner * esize;
    p.n_inner = (uint32_t)v->n_inner;
    p.on = 1;
    return true;
}

// the shared check lists below return CONTINUE where the entry point goes on; any other value is the entry point's result
constexpr int CONTINUE = 1;

// what rowwise<> and fq_sym_fwd_autocast check first, behind their own dtype check (named: the site's wording of a negative shape)
int fwd_head(const void* x, const void* y, int64_t rows, int64_t cols, int bits, int sem, bool named) {
    if (bits < 1 || bits > 31) return fail(FQ_ERR_BITS, "num_bits=%d outside [1, 31]", bits);
    if (sem != FQ_SEM_CPU_EAGER && sem != FQ_SEM_DEVICE_EAGER) return fail(FQ_ERR_ARG, "unknown semantics code %d", sem);
    if (rows < 0 || cols < 0)
        return named ? fail(FQ_ERR_SHAPE, "negative shape rows=%lld cols=%lld", (long long)rows, (long long)cols) : fail(FQ_ERR_SHAPE, "negative shape");
    if (rows == 0 || cols == 0) return ok();  // empty tensor: nothing to do (the reference returns an empty tensor)
    if (!x || !y) return fail(FQ_ERR_NULL, "x / y must not be NULL");
    if (x == y) return fail(FQ_ERR_ARG, "in-place (y == x) is not supported");
    return CONTINUE;
}

// The checks every MX entry point makes, in the order they run: the dtype, `first` (the entry point's own: formats, flags), the shape,
// `pointers` (its own: NULL, aliasing, alignment), the launch's size.  Both callables return 0 or their refusal.  CONTINUE with nvec (the
// tensor in 16-byte vectors) set, or the entry point's result.  Every check comes before any HIP call.
template <class First, class Pointers>
int mx_checks(int dtype, int64_t rows, int64_t cols, bool rot, int64_t& nvec, First&& first, Pointers&& pointers) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the MX entry points");
    if (const int rc = first()) return rc;
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (rot && cols % MX_ROT_RUN != 0) return fail(FQ_ERR_SHAPE, "cols=%lld is not a multiple of the %d-element rotation run", (long long)cols, MX_ROT_RUN);
    if (cols % 32 != 0) return fail(FQ_ERR_SHAPE, "cols=%lld is not a multiple of the 32-element MX block", (long long)cols);
    if (cols > 0 && rows > INT64_MAX / 4 / cols) return fail(FQ_ERR_SHAPE, "rows * cols overflows");
    if (rows == 0 || cols == 0) return ok();
    if (const int rc = pointers()) return rc;
    nvec = rows * cols * esize_of(dtype) / 16;    // cols % 32 == 0: whole 16-byte vectors, whole blocks
    if (nvec / (MX_TPB * MX_VPT) >= 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "%lld vectors exceed one launch's grid", (long long)nvec);
    return CONTINUE;
}

// the `pointers` of an MX entry point that reads x and writes y: 0 or the refusal
int mx_xy_pointers(const void* x, const void* y) {
    if (!x || !y) return fail(FQ_ERR_NULL, "x / y must not be NULL");
    if (x == y) return fail(FQ_ERR_ARG, "in-place (y == x) is not supported");
    if (!aligned16(x) || !aligned16(y)) return fail(FQ_ERR_UNSUPPORTED, "pointers must be 16-byte aligned");
    return 0;
}

template <bool ASYM>
int rowwise(const void* x, void* y, int32_t* idx, float* scale, float* bounds, int64_t rows, int64_t cols, int bits, int dtype,
            int sem, void* ws, size_t wsb, void* stream, const MaskArgs* mk = nullptr, const fq_rows_view* xv = nullptr,
            const fq_rows_view* yv = nullptr) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (const int rc = fwd_head(x, y, rows, cols, bits, sem, true); rc != CONTINUE) return rc;
    if (dtype == FQ_DTYPE_F64) {  // correctness path in double arithmetic; no training-mode side buffers
        if (bounds || mk) return fail(FQ_ERR_DTYPE, "float64 tensors: row bounds / STE mask are not produced (use fq_ste_bwd, the reference's data flow)");
        if ((xv && xv->n_inner > 0) || (yv && yv->n_inner > 0)) return fail(FQ_ERR_UNSUPPORTED, "float64 tensors: contiguous rows only");
        return launch_f64_rowwise(ASYM, x, y, idx, scale, rows, cols, bits, sem, (hipStream_t)stream);
    }
    const Consts c = make_consts(bits, dtype, sem);
    RowArgs a{x, y, idx, scale, bounds, rows, cols, c.sym, c.asym, nullptr, 0, 0.f, 0.f, 0u, rows, 0, {}};
    if (!set_pitch(a.xp, xv, rows, cols, esize_of(dtype)) || !set_pitch(a.yp, yv, rows, cols, esize_of(dtype)))
        return fail(FQ_ERR_SHAPE, "fq_rows_view: negative stride, or more than 2^31 - 1 rows");
    if (mk) {
        if (!mk->mask || !bounds) return fail(FQ_ERR_NULL, "train-mode forward needs row_bounds_out and mask_out");
        if (const int rc = set_mask_args(a, mk->mask, mk->bytes, mk->lo, mk->hi, dtype)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    // reciprocal-multiply instead of IEEE divide (only honoured for bf16).  Sym: valid for every bit width, because
    // the bin index is rint() of a bf16 value and so has an 8-bit significand itself; Asym: the divisor 2^bits-1 must
    // have one too, i.e. bits <= 8.
    const bool fast = ASYM ? bits <= 8 : true;
    return by_dtype(dtype, [&](auto dt) { return launch_rowwise<decltype(dt)::value>(ASYM, fast, a, ws, wsb, st); });
}

}  // namespace

#define FQ_API __attribute__((visibility("default")))

extern "C" {

FQ_API int fq_version(void) { return FQ_ABI_VERSION; }

FQ_API const char* fq_build_info(void) {
    static char buf[160];
    snprintf(buf, sizeof(buf), "llmqat_fakequant abi %d, gfx950 (CDNA4, wave64), HIP %d.%d, -ffp-contract=off", FQ_ABI_VERSION,
             HIP_VERSION_MAJOR, HIP_VERSION_MINOR);
    return buf;
}

FQ_API const char* fq_last_error(void) { return g_err; }

FQ_API size_t fq_rowwise_workspace_bytes(int64_t rows, int64_t cols, int dtype) {
    (void)dtype;
    if (rows <= 0 || cols <= WS_COLS_THRESHOLD) return 0;
    return (size_t)rows * 8;
}

FQ_API int fq_sym_fwd(const void* x, void* y, int64_t rows, int64_t cols, int bits, int dtype, int sem, float* row_bounds_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
    return rowwise<false>(x, y, nullptr, nullptr, row_bounds_out, rows, cols, bits, dtype, sem, workspace, workspace_bytes, stream);
}
FQ_API int fq_asym_fwd(const void* x, void* y, int64_t rows, int64_t cols, int bits, int dtype, int sem, float* row_bounds_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    return rowwise<true>(x, y, nullptr, nullptr, row_bounds_out, rows, cols, bits, dtype, sem, workspace, workspace_bytes, stream);
}
FQ_API int fq_sym_fwd_debug(const void* x, void* y, int32_t* idx_out, float* scale_out, int64_t rows, int64_t cols, int bits,
                            int dtype, int sem, void* workspace, size_t workspace_bytes, void* stream) {
    return rowwise<false>(x, y, idx_out, scale_out, nullptr, rows, cols, bits, dtype, sem, workspace, workspace_bytes, stream);
}
FQ_API int fq_asym_fwd_debug(const void* x, void* y, int32_t* idx_out, float* scale_out, int64_t rows, int64_t cols, int bits,
                             int dtype, int sem, void* workspace, size_t workspace_bytes, void* stream) {
    return rowwise<true>(x, y, idx_out, scale_out, nullptr, rows, cols, bits, dtype, sem, workspace, workspace_bytes, stream);
}

FQ_API size_t fq_ste_mask_bytes(int64_t rows, int64_t cols, int dtype) {
    if (dtype < 0 || dtype > 2 || rows <= 0) return 0;
    return (size_t)rows * (size_t)mask_row_words(cols, esize_of(dtype)) * 8;
}

FQ_API int fq_sym_fwd_train(const void* x, void* y, int64_t rows, int64_t cols, int bits, int dtype, int sem, float lo, float hi,
                            float* row_bounds_out, void* mask_out, size_t mask_bytes, void* stream) {
    const MaskArgs mk{mask_out, mask_bytes, lo, hi};
    return rowwise<false>(x, y, nullptr, nullptr, row_bounds_out, rows, cols, bits, dtype, sem, nullptr, 0, stream, &mk);
}
FQ_API int fq_asym_fwd_train(const void* x, void* y, int64_t rows, int64_t cols, int bits, int dtype, int sem, float lo, float hi,
                             float* row_bounds_out, void* mask_out, size_t mask_bytes, void* stream) {
    const MaskArgs mk{mask_out, mask_bytes, lo, hi};
    return rowwise<true>(x, y, nullptr, nullptr, row_bounds_out, rows, cols, bits, dtype, sem, nullptr, 0, stream, &mk);
}

FQ_API int fq_sym_fwd_autocast(const void* x, void* y, int64_t rows, int64_t cols, int bits, int dtype, int sem, int wide_out, float lo, float hi,
                               float* row_bounds_out, void* mask_out, size_t mask_bytes, void* workspace, size_t workspace_bytes,
                               void* stream) {
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16)
        return fail(FQ_ERR_DTYPE, "autocast arithmetic applies to bf16 / fp16 tensors (fp32 tensors are unaffected by autocast)");
    if (const int rc = fwd_head(x, y, rows, cols, bits, sem, false); rc != CONTINUE) return rc;
    const Consts c = make_consts(bits, dtype, sem);  // under autocast `sem` touches `max + 1e-6` only (everything behind it is fp32)
    RowArgs a{x, y, nullptr, nullptr, row_bounds_out, rows, cols, c.sym, c.asym, nullptr, 0, 0.f, 0.f, 0u, rows, 0, {}};
    if (mask_out) {
        if (!row_bounds_out) return fail(FQ_ERR_NULL, "a mask needs row_bounds_out too");
        if (const int rc = set_mask_args(a, mask_out, mask_bytes, lo, hi, dtype)) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_sym_autocast<decltype(dt)::value>(wide_out != 0, a, workspace, workspace_bytes, st); });
}

static int sym_fwd_multi_impl(int n, const fq_fwd_tensor* t, const fq_rows_view* const* xv, const fq_rows_view* const* yv, int64_t cols, int dtype,
                              int sem, int autocast, float lo, float hi, void* stream) {
    if (dtype < 0 || dtype > 2) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (n < 1 || n > 1 + MAX_MORE || !t) return fail(FQ_ERR_ARG, "a launch takes 1 to %d tensors", 1 + MAX_MORE);
    if (sem != FQ_SEM_CPU_EAGER && sem != FQ_SEM_DEVICE_EAGER) return fail(FQ_ERR_ARG, "unknown semantics code %d", sem);
    if (autocast < 0 || autocast > 2) return fail(FQ_ERR_ARG, "autocast must be 0, 1 or 2");
    if (autocast && dtype == FQ_DTYPE_F32) return fail(FQ_ERR_DTYPE, "autocast arithmetic applies to bf16 / fp16 tensors only");
    if (cols <= 0) return fail(FQ_ERR_SHAPE, "multi-tensor launch needs non-empty tensors");
    const int64_t mrw = mask_row_words(cols, esize_of(dtype));
    if (!mrw) return fail(FQ_ERR_UNSUPPORTED, "shape not served by the register kernels (see fq_ste_mask_bytes)");
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (t[i].bits < 1 || t[i].bits > 31) return fail(FQ_ERR_BITS, "num_bits outside [1, 31]");
        if (t[i].rows <= 0) return fail(FQ_ERR_SHAPE, "multi-tensor launch needs non-empty tensors");
        if (!t[i].x || !t[i].y) return fail(FQ_ERR_NULL, "multi-tensor launch: x / y of every tensor required");
        if (t[i].mask && !t[i].row_bounds) return fail(FQ_ERR_NULL, "a mask needs its row_bounds too");
        if (t[i].mask && t[i].mask_bytes < (size_t)t[i].rows * mrw * 8) return fail(FQ_ERR_WORKSPACE, "mask buffer too small");
        total += t[i].rows;
    }
    const Consts c0 = make_consts(t[0].bits, dtype, sem);
    RowArgs a{t[0].x, t[0].y, nullptr, nullptr, t[0].row_bounds, total, cols, c0.sym, c0.asym, (uint64_t*)t[0].mask, mrw, host_rb(lo, dtype),
              host_rb(hi, dtype), ste_clip_key(host_rb(lo, dtype), host_rb(hi, dtype), dtype), t[0].rows, n - 1, {}};
    int64_t begin = t[0].rows;
    for (int i = 1; i < n; ++i) {
        a.more[i - 1] = TensorSlot{begin, t[i].x, t[i].y, t[i].row_bounds, (uint64_t*)t[i].mask, make_consts(t[i].bits, dtype, sem).sym.qmax, {}, {}};
        begin += t[i].rows;
    }
    {   // rows that do not follow one another (the _v entry point); the results of an autocast = 2 launch are fp32
        const int xe = esize_of(dtype), ye = autocast == 2 ? 4 : xe;
        bool okv = true;
        for (int i = 0; i < n; ++i) {
            RowPitch& px = i ? a.more[i - 1].xp : a.xp;
            RowPitch& py = i ? a.more[i - 1].yp : a.yp;
            okv = okv && set_pitch(px, xv ? xv[i] : nullptr, t[i].rows, cols, xe) && set_pitch(py, yv ? yv[i] : nullptr, t[i].rows, cols, ye);
        }
        if (!okv) return fail(FQ_ERR_SHAPE, "fq_rows_view: negative stride, or more than 2^31 - 1 rows");
    }
    hipStream_t st = (hipStream_t)stream;
    if (autocast) {
        const bool wide = autocast == 2;  // the y are fp32; masks (if any) in the wide layout, for fq_ste_bwd_mask_wide
        return by_dtype(dtype, [&](auto dt) { return launch_sym_autocast<decltype(dt)::value>(wide, a, nullptr, 0, st); });
    }
    return by_dtype(dtype, [&](auto dt) { return launch_rowwise<decltype(dt)::value>(false, true, a, nullptr, 0, st); });
}

FQ_API int fq_sym_fwd_multi(int n, const fq_fwd_tensor* t, int64_t cols, int dtype, int sem, int autocast, float lo, float hi, void* stream) {
    return sym_fwd_multi_impl(n, t, nullptr, nullptr, cols, dtype, sem, autocast, lo, hi, stream);
}

FQ_API int fq_sym_fwd_multi_v(int n, const fq_fwd_tensor_v* tv, int64_t cols, int dtype, int sem, int autocast, float lo, float hi, void* stream) {
    if (n < 1 || n > 1 + MAX_MORE || !tv) return fail(FQ_ERR_ARG, "a launch takes 1 to %d tensors", 1 + MAX_MORE);
    fq_fwd_tensor t[1 + MAX_MORE];
    const fq_rows_view *xv[1 + MAX_MORE], *yv[1 + MAX_MORE];
    for (int i = 0; i < n; ++i) {
        t[i] = fq_fwd_tensor{tv[i].x, tv[i].y, tv[i].rows, tv[i].bits, tv[i].row_bounds, tv[i].mask, tv[i].mask_bytes};
        xv[i] = &tv[i].xv;
        yv[i] = &tv[i].yv;
    }
    return sym_fwd_multi_impl(n, t, xv, yv, cols, dtype, sem, autocast, lo, hi, stream);
}

FQ_API int fq_rowwise_fwd_v(int asym, const void* x, const fq_rows_view* xv, void* y, const fq_rows_view* yv, int64_t rows, int64_t cols, int bits,
                            int dtype, int sem, float lo, float hi, float* row_bounds_out, void* mask_out, size_t mask_bytes, void* stream) {
    const MaskArgs mk{mask_out, mask_bytes, lo, hi};
    const MaskArgs* m = mask_out ? &mk : nullptr;
    return asym ? rowwise<true>(x, y, nullptr, nullptr, row_bounds_out, rows, cols, bits, dtype, sem, nullptr, 0, stream, m, xv, yv)
                : rowwise<false>(x, y, nullptr, nullptr, row_bounds_out, rows, cols, bits, dtype, sem, nullptr, 0, stream, m, xv, yv);
}

FQ_API int fq_sym_fwd_pair(const void* x0, void* y0, int64_t rows0, int bits0, float* row_bounds0, void* mask0, size_t mask_bytes0,
                           const void* x1, void* y1, int64_t rows1, int bits1, float* row_bounds1, void* mask1, size_t mask_bytes1,
                           int64_t cols, int dtype, int sem, int autocast, float lo, float hi, void* stream) {
    const fq_fwd_tensor t[2] = {{x0, y0, rows0, bits0, row_bounds0, mask0, mask_bytes0}, {x1, y1, rows1, bits1, row_bounds1, mask1, mask_bytes1}};
    return fq_sym_fwd_multi(2, t, cols, dtype, sem, autocast, lo, hi, stream);
}

static int ste_bwd_mask_multi_impl(int n, const fq_bwd_tensor* t, const fq_rows_view* const* gv, const fq_rows_view* const* ov, int64_t cols, float lo,
                                   float hi, int dtype, int wide_grad, void* stream) {
    if (dtype < 0 || dtype > 2) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (wide_grad && dtype == FQ_DTYPE_F32) return fail(FQ_ERR_DTYPE, "fp32-gradient STE backward: the input dtype must be bf16 / fp16");
    if (n < 1 || n > 1 + MAX_MORE || !t) return fail(FQ_ERR_ARG, "a launch takes 1 to %d tensors", 1 + MAX_MORE);
    if (cols <= 0) return fail(FQ_ERR_SHAPE, "multi-tensor launch needs non-empty tensors");
    if (!mask_row_words(cols, esize_of(dtype))) return fail(FQ_ERR_UNSUPPORTED, "shape not served by the STE-mask path");
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (t[i].rows <= 0) return fail(FQ_ERR_SHAPE, "multi-tensor launch needs non-empty tensors");
        if (!t[i].g || !t[i].gx || !t[i].row_bounds || !t[i].mask) return fail(FQ_ERR_NULL, "multi-tensor launch: all buffers required");
        total += t[i].rows;
    }
    lo = host_rb(lo, dtype);
    hi = host_rb(hi, dtype);
    SteLaunch L{};
    L.n = n;
    for (int i = 0; i < n; ++i) {
        L.t[i] = SteSlot{t[i].g, t[i].gx, t[i].row_bounds, (const uint64_t*)t[i].mask, t[i].rows, 0, 0, {}, {}};
        const int oe = esize_of(dtype), ge = wide_grad ? 4 : oe;   // behind a fp32-result forward the gradient is fp32
        if (!set_pitch(L.t[i].gp, gv ? gv[i] : nullptr, t[i].rows, cols, ge) || !set_pitch(L.t[i].op, ov ? ov[i] : nullptr, t[i].rows, cols, oe))
            return fail(FQ_ERR_SHAPE, "fq_rows_view: negative stride, or more than 2^31 - 1 rows");
        if (t[i].gx == (const void*)t[i].g && memcmp(&L.t[i].gp, &L.t[i].op, sizeof(RowPitch)) != 0)
            return fail(FQ_ERR_ARG, "an in-place tensor (gx == g) needs equal views");
    }
    hipStream_t st = (hipStream_t)stream;
    if (wide_grad) return by_dtype(dtype, [&](auto dt) { return launch_ste_mask_wide<decltype(dt)::value>(L, cols, lo, hi, st); });
    return by_dtype(dtype, [&](auto dt) { return launch_ste_mask<decltype(dt)::value>(L, cols, lo, hi, st); });
}

FQ_API int fq_ste_bwd_mask_multi(int n, const fq_bwd_tensor* t, int64_t cols, float lo, float hi, int dtype, int wide_grad, void* stream) {
    return ste_bwd_mask_multi_impl(n, t, nullptr, nullptr, cols, lo, hi, dtype, wide_grad, stream);
}

FQ_API int fq_ste_bwd_mask_multi_v(int n, const fq_bwd_tensor_v* tv, int64_t cols, float lo, float hi, int dtype, int wide_grad, void* stream) {
    if (n < 1 || n > 1 + MAX_MORE || !tv) return fail(FQ_ERR_ARG, "a launch takes 1 to %d tensors", 1 + MAX_MORE);
    fq_bwd_tensor t[1 + MAX_MORE];
    const fq_rows_view *gv[1 + MAX_MORE], *ov[1 + MAX_MORE];
    for (int i = 0; i < n; ++i) {
        t[i] = fq_bwd_tensor{tv[i].g, tv[i].gx, tv[i].rows, tv[i].row_bounds, tv[i].mask};
        gv[i] = &tv[i].gv;
        ov[i] = &tv[i].gxv;
    }
    return ste_bwd_mask_multi_impl(n, t, gv, ov, cols, lo, hi, dtype, wide_grad, stream);
}

FQ_API int fq_ste_bwd_mask_pair(const void* g0, void* gx0, int64_t rows0, const float* row_bounds0, const void* mask0,
                                const void* g1, void* gx1, int64_t rows1, const float* row_bounds1, const void* mask1,
                                int64_t cols, float lo, float hi, int dtype, void* stream) {
    const fq_bwd_tensor t[2] = {{g0, gx0, rows0, row_bounds0, mask0}, {g1, gx1, rows1, row_bounds1, mask1}};
    return fq_ste_bwd_mask_multi(2, t, cols, lo, hi, dtype, 0, stream);
}

FQ_API int fq_ste_bwd_mask_wide(const void* g0, void* gx0, int64_t rows0, const float* row_bounds0, const void* mask0,
                                const void* g1, void* gx1, int64_t rows1, const float* row_bounds1, const void* mask1,
                                int64_t cols, float lo, float hi, int dtype, void* stream) {
    if (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16) return fail(FQ_ERR_DTYPE, "fp32-gradient STE backward: the input dtype must be bf16 / fp16");
    if (rows0 < 0 || rows1 < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape");
    if ((rows0 == 0 && rows1 == 0) || cols == 0) return ok();
    if (rows0 == 0) return fail(FQ_ERR_SHAPE, "a single tensor goes first (rows1 = 0)");
    const fq_bwd_tensor t[2] = {{g0, gx0, rows0, row_bounds0, mask0}, {g1, gx1, rows1, row_bounds1, mask1}};
    return fq_ste_bwd_mask_multi(rows1 ? 2 : 1, t, cols, lo, hi, dtype, 1, stream);
}

FQ_API int fq_ste_bwd_mask(const void* g, void* gx, int64_t rows, int64_t cols, float lo, float hi, const float* row_bounds,
                           const void* mask, size_t mask_bytes, int dtype, void* stream) {
    if (dtype < 0 || dtype > 2) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape");
    if (rows == 0 || cols == 0) return ok();
    if (!g || !gx || !row_bounds || !mask) return fail(FQ_ERR_NULL, "g / gx / row_bounds / mask must not be NULL");
    const int64_t mrw = mask_row_words(cols, esize_of(dtype));
    if (!mrw) return fail(FQ_ERR_UNSUPPORTED, "shape not served by the STE-mask path (see fq_ste_mask_bytes)");
    if (mask_bytes < (size_t)rows * mrw * 8) return fail(FQ_ERR_WORKSPACE, "mask buffer too small");
    const fq_bwd_tensor t{g, gx, rows, row_bounds, mask};
    return fq_ste_bwd_mask_multi(1, &t, cols, lo, hi, dtype, 0, stream);
}

FQ_API int fq_w12_fwd(const void* w, const void* scale, void* out, int64_t rows, int64_t cols, int w_bits, int scale_per_row,
                      int dtype, void* stream) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (w_bits != 1 && w_bits != 2) return fail(FQ_ERR_BITS, "w_bits=%d: this entry point serves 1 and 2", w_bits);
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape");
    if (rows == 0 || cols == 0) return ok();
    if (!w || !scale || !out) return fail(FQ_ERR_NULL, "w / scale / out must not be NULL");
    if (dtype == FQ_DTYPE_F64) return launch_f64_w12(w, scale, out, rows, cols, w_bits, scale_per_row, (hipStream_t)stream);
    // clip_val = 1 - 1e-2 (utils_quant.py:217): a Python double; the clamp compares in fp32 on the device and in the
    // tensor dtype on the CPU -- both give the same results (DESIGN.md "Numerics"), fp32 is used here
    const float cv = (float)(1.0 - 1e-2);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_w12<decltype(dt)::value>(w, scale, out, rows, cols, w_bits, scale_per_row, cv, st); });
}

FQ_API int fq_w12_fwd_rows(const void* w, void* out, void* scale_out, int64_t rows, int64_t cols, int w_bits, int dtype, void* stream) {
    if (dtype < 0 || dtype > 2) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (w_bits != 1 && w_bits != 2) return fail(FQ_ERR_BITS, "w_bits=%d: this entry point serves 1 and 2", w_bits);
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape");
    if (rows == 0 || cols == 0) return ok();
    if (!w || !out) return fail(FQ_ERR_NULL, "w / out must not be NULL");
    const float cv = (float)(1.0 - 1e-2);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_w12_rows<decltype(dt)::value>(w, out, scale_out, rows, cols, w_bits, cv, st); });
}

FQ_API int fq_ste_bwd(const void* g, const void* x, void* gx, int64_t n, float lo, float hi, int dtype, void* stream) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (n < 0) return fail(FQ_ERR_SHAPE, "negative n");
    if (n == 0) return ok();
    if (!g || !x || !gx) return fail(FQ_ERR_NULL, "g / x / gx must not be NULL");
    if (dtype == FQ_DTYPE_F64) return launch_f64_ste(g, x, gx, n, lo, hi, (hipStream_t)stream);  // the clip is a float32 tensor (:198,:245): its values as doubles
    lo = host_rb(lo, dtype);  // the reference compares in the tensor dtype (utils_quant.py:85-86)
    hi = host_rb(hi, dtype);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_ste<decltype(dt)::value>(g, x, gx, n, lo, hi, st); });
}

FQ_API int fq_ste_bwd_rows(const void* g, const void* x, void* gx, int64_t rows, int64_t cols, float lo, float hi,
                           const float* row_bounds, int dtype, void* stream) {
    if (dtype < 0 || dtype > 2) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape");
    if (rows == 0 || cols == 0) return ok();
    if (!g || !x || !gx || !row_bounds) return fail(FQ_ERR_NULL, "g / x / gx / row_bounds must not be NULL");
    lo = host_rb(lo, dtype);
    hi = host_rb(hi, dtype);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_ste_rows<decltype(dt)::value>(g, x, gx, rows, cols, lo, hi, row_bounds, st); });
}

FQ_API int fq_ste_bwd_v(const void* g, const fq_rows_view* gv, const void* x, const fq_rows_view* xv, void* gx, const fq_rows_view* gxv, int64_t rows,
                        int64_t cols, float lo, float hi, const float* row_bounds, int dtype, void* stream) {
    if (dtype < 0 || dtype > 2) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape");
    if (rows == 0 || cols == 0) return ok();
    if (!g || !x || !gx) return fail(FQ_ERR_NULL, "g / x / gx must not be NULL");
    StePitch3 p{};
    const int es = esize_of(dtype);
    if (!set_pitch(p.g, gv, rows, cols, es) || !set_pitch(p.x, xv, rows, cols, es) || !set_pitch(p.o, gxv, rows, cols, es))
        return fail(FQ_ERR_SHAPE, "fq_rows_view: negative stride, or more than 2^31 - 1 rows");
    lo = host_rb(lo, dtype);
    hi = host_rb(hi, dtype);
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_ste_rows<decltype(dt)::value>(g, x, gx, rows, cols, lo, hi, row_bounds, st, p); });
}

FQ_API int fq_group_fwd(int asym, const void* x, void* y, int64_t rows, int64_t cols, int64_t group, int bits, int dtype, int sem, int autocast,
                        float lo, float hi, float* row_bounds_out, void* mask_out, size_t mask_bytes, void* stream) {
    // every check comes before any division or launch (the ABI fuzz passes group = 0, negatives and 2^62)
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (asym != 0 && asym != 1) return fail(FQ_ERR_ARG, "asym must be 0 or 1");
    if (bits < 1 || bits > 31) return fail(FQ_ERR_BITS, "num_bits=%d outside [1, 31]", bits);
    if (sem != FQ_SEM_CPU_EAGER && sem != FQ_SEM_DEVICE_EAGER) return fail(FQ_ERR_ARG, "unknown semantics code %d", sem);
    if (autocast != 0 && autocast != 1) return fail(FQ_ERR_ARG, "autocast must be 0 or 1 (the fp32-result form is not served here)");
    if (autocast && (asym || (dtype != FQ_DTYPE_BF16 && dtype != FQ_DTYPE_F16)))
        return fail(FQ_ERR_DTYPE, "autocast arithmetic applies to SymQuantizer on bf16 / fp16 tensors only");
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (group <= 0) return fail(FQ_ERR_ARG, "group=%lld must be positive", (long long)group);
    if (cols % group != 0) return fail(FQ_ERR_SHAPE, "group=%lld does not divide cols=%lld", (long long)group, (long long)cols);
    if (cols > 0 && rows > INT64_MAX / cols) return fail(FQ_ERR_SHAPE, "rows * cols overflows");
    if (rows == 0 || cols == 0) return ok();
    if (!x || !y) return fail(FQ_ERR_NULL, "x / y must not be NULL");
    if (x == y) return fail(FQ_ERR_ARG, "in-place (y == x) is not supported");
    if (mask_out && !row_bounds_out) return fail(FQ_ERR_NULL, "a mask needs row_bounds_out too");
    if (dtype == FQ_DTYPE_F64) return fail(FQ_ERR_UNSUPPORTED, "float64: quantize the [rows * cols / group, group] view with fq_sym_fwd / fq_asym_fwd");
    const int es = esize_of(dtype), epv = 16 / es;
    if (cols / epv > REG_MAX_VEC) return fail(FQ_ERR_UNSUPPORTED, "rows longer than %lld vectors are not served", (long long)REG_MAX_VEC);
    const int64_t gbytes = group * es;   // group <= cols <= 8 * REG_MAX_VEC: no overflow
    const int64_t gv = gbytes / 16;
    if (gbytes % 16 != 0 || !(gv == 4 || gv == 8 || gv == 16 || gv == 32 || gv == 64))
        return fail(FQ_ERR_UNSUPPORTED, "group=%lld: the kernel serves groups of 4..64 16-byte vectors (bf16 / fp16 g = 32..512, fp32 g = 16..256)", (long long)group);
    if (rows > 0x7FFFFFFF) return fail(FQ_ERR_UNSUPPORTED, "rows=%lld exceeds the grid limit", (long long)rows);
    if (!aligned16(x) || !aligned16(y)) return fail(FQ_ERR_UNSUPPORTED, "x / y must be 16-byte aligned");
    const Consts c = make_consts(bits, dtype, sem);
    RowArgs a{x, y, nullptr, nullptr, row_bounds_out, rows, cols, c.sym, c.asym, nullptr, 0, 0.f, 0.f, 0u, rows, 0, {}};
    if (mask_out) {   // (the shape is served: whole vectors and at most REG_MAX_VEC of them, checked above)
        if (const int rc = set_mask_args(a, mask_out, mask_bytes, lo, hi, dtype)) return rc;
    }
    seal_slots(a);
    hipStream_t st = (hipStream_t)stream;
    const bool fast = asym ? bits <= 8 : true;   // as rowwise(): only bf16 honours it
    return by_dtype(dtype, [&](auto dt) { return launch_group<decltype(dt)::value>(asym != 0, fast, autocast, a, (int)gv, st); });   // fp32: autocast == 0
}

namespace {
// element formats of the MX entry points, indexed by FQ_MX_*: {emax, mbits, emin, max-normal, code of max-normal, sign bit of a code}
const MxFmt kMxFmts[5] = {
    {2, 1, 0, 6.0f, 0x7u, 0x8u},            // E2M1
    {2, 3, 0, 7.5f, 0x1Fu, 0x20u},          // E2M3
    {4, 2, -2, 28.0f, 0x1Fu, 0x20u},        // E3M2
    {8, 3, -6, 448.0f, 0x7Eu, 0x80u},       // E4M3 (0x7F is its NaN)
    {15, 2, -14, 57344.0f, 0x7Bu, 0x80u},   // E5M2
};

// exp = false: fq_mx_fwd (x -> y); true: fq_mx_export (x -> elems + scales).  rot: the *_rot forms (x R is quantized); only_rot:
// fq_block_rotate (x -> y = x R, no format).  ceil: the scale rule of the *_ex forms; mask (forward only, optional): the saturation
// bitmap, rows * cols / 8 bytes.
int mx_entry(bool exp, const void* x, void* y, void* elems, void* scales, int64_t rows, int64_t cols, int fmt, int dtype, void* stream,
             bool rot = false, bool only_rot = false, bool ceil = false, void* mask = nullptr) {
    auto formats = [&] {
        if (!only_rot && (fmt < FQ_MX_FP4_E2M1 || fmt > FQ_MX_FP8_E5M2)) return fail(FQ_ERR_ARG, "unknown MX format code %d", fmt);
        if (exp && (fmt == FQ_MX_FP6_E2M3 || fmt == FQ_MX_FP6_E3M2)) return fail(FQ_ERR_ARG, "FP6 formats have no export packing");
        return 0;
    };
    auto pointers = [&] {
        if (!x || (!exp && !y) || (exp && (!elems || !scales))) return fail(FQ_ERR_NULL, exp ? "x / elems / scales must not be NULL" : "x / y must not be NULL");
        if (!exp && x == y) return fail(FQ_ERR_ARG, "in-place (y == x) is not supported");
        if (mask && (mask == x || mask == y)) return fail(FQ_ERR_ARG, "mask_out must not alias x or y");
        if (!aligned16(x) || (!exp && !aligned16(y)) || (exp && (!aligned16(elems) || !aligned16(scales))) || !aligned16(mask))
            return fail(FQ_ERR_UNSUPPORTED, "pointers must be 16-byte aligned");
        return 0;
    };
    int64_t nvec = 0;
    if (const int rc = mx_checks(dtype, rows, cols, rot, nvec, formats, pointers); rc != CONTINUE) return rc;
    MxArgs a{x, y, (uint8_t*)(mask ? mask : elems), (uint8_t*)scales, nvec, nvec * 16 >= NT_LOAD_MIN_BYTES ? 1 : 0};
    const int kind = only_rot ? MX_ROT : !exp ? MX_FWD : (fmt == FQ_MX_FP4_E2M1 ? MX_EXP4 : MX_EXP8);
    hipStream_t st = (hipStream_t)stream;
    const MxFmt& f = kMxFmts[only_rot ? 0 : fmt];
    return by_dtype(dtype, [&](auto dt) { return launch_mx<decltype(dt)::value>(kind, rot, ceil, mask != nullptr, a, f, st); });
}
const int kMxFlags = FQ_MX_FLAG_ROTATE | FQ_MX_FLAG_CEIL;
}  // namespace

FQ_API int fq_mx_fwd(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, void* stream) {
    return mx_entry(false, x, y, nullptr, nullptr, rows, cols, fmt, dtype, stream);
}

FQ_API int fq_mx_export(const void* x, void* elems_out, void* scales_out, int64_t rows, int64_t cols, int fmt, int dtype, void* stream) {
    return mx_entry(true, x, nullptr, elems_out, scales_out, rows, cols, fmt, dtype, stream);
}

FQ_API int fq_mx_fwd_rot(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, void* stream) {
    return mx_entry(false, x, y, nullptr, nullptr, rows, cols, fmt, dtype, stream, true);
}

FQ_API int fq_mx_export_rot(const void* x, void* elems_out, void* scales_out, int64_t rows, int64_t cols, int fmt, int dtype, void* stream) {
    return mx_entry(true, x, nullptr, elems_out, scales_out, rows, cols, fmt, dtype, stream, true);
}

FQ_API int fq_block_rotate(const void* x, void* y, int64_t rows, int64_t cols, int dtype, void* stream) {
    return mx_entry(false, x, y, nullptr, nullptr, rows, cols, 0, dtype, stream, true, true);
}

FQ_API int fq_mx_fwd_ex(const void* x, void* y, void* mask_out, int64_t rows, int64_t cols, int fmt, int dtype, int flags, void* stream) {
    if (flags & ~kMxFlags) return fail(FQ_ERR_ARG, "unknown flag bits 0x%x", (unsigned)(flags & ~kMxFlags));
    return mx_entry(false, x, y, nullptr, nullptr, rows, cols, fmt, dtype, stream, (flags & FQ_MX_FLAG_ROTATE) != 0, false,
                    (flags & FQ_MX_FLAG_CEIL) != 0, mask_out);
}

FQ_API int fq_mx_export_ex(const void* x, void* elems_out, void* scales_out, int64_t rows, int64_t cols, int fmt, int dtype, int flags,
                           void* stream) {
    if (flags & ~kMxFlags) return fail(FQ_ERR_ARG, "unknown flag bits 0x%x", (unsigned)(flags & ~kMxFlags));
    return mx_entry(true, x, nullptr, elems_out, scales_out, rows, cols, fmt, dtype, stream, (flags & FQ_MX_FLAG_ROTATE) != 0, false,
                    (flags & FQ_MX_FLAG_CEIL) != 0);
}

// gx == g is served without the rotation (every lane stores the vector it loaded).
FQ_API int fq_mx_ste_bwd(const void* g, const void* mask, void* gx, int64_t rows, int64_t cols, int dtype, int flags, void* stream) {
    const bool rot = (flags & FQ_MX_FLAG_ROTATE) != 0;
    auto flag_bits = [&] {
        if (flags & ~FQ_MX_FLAG_ROTATE) return fail(FQ_ERR_ARG, "flag bits 0x%x: the backward takes FQ_MX_FLAG_ROTATE only", (unsigned)(flags & ~FQ_MX_FLAG_ROTATE));
        return 0;
    };
    auto pointers = [&] {
        if (!g || !mask || !gx) return fail(FQ_ERR_NULL, "g / mask / gx must not be NULL");
        if (mask == g || mask == gx) return fail(FQ_ERR_ARG, "mask must not alias g or gx");
        if (rot && g == gx) return fail(FQ_ERR_ARG, "in-place (gx == g) is not supported with the rotation");
        if (!aligned16(g) || !aligned16(mask) || !aligned16(gx)) return fail(FQ_ERR_UNSUPPORTED, "pointers must be 16-byte aligned");
        return 0;
    };
    int64_t nvec = 0;
    if (const int rc = mx_checks(dtype, rows, cols, rot, nvec, flag_bits, pointers); rc != CONTINUE) return rc;
    const MxSteArgs a{g, (const uint32_t*)mask, gx, nvec, nvec * 16 >= NT_LOAD_MIN_BYTES ? 1 : 0};
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_mx_ste<decltype(dt)::value>(rot, a, st); });
}

namespace {
// The checks of the column-axis entry points (fqt_mx_fwd_cols, fqs_mx_fwd_cols): mx_checks' in mx_checks' order, with the block along the
// rows: rows % 32 in place of cols % 32, whole 16-byte strips per row, and the grid counted in tiles.  CONTINUE with a and row_tiles set,
// or the entry point's result.  Every check comes before any HIP call.
int mx_cols_checks(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, int flags, MxColsArgs& a, int64_t& row_tiles) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the MX entry points");
    if (fmt < FQ_MX_FP4_E2M1 || fmt > FQ_MX_FP8_E5M2) return fail(FQ_ERR_ARG, "unknown MX format code %d", fmt);
    if (flags & ~FQ_MX_FLAG_CEIL) return fail(FQ_ERR_ARG, "flag bits 0x%x: the column axis takes FQ_MX_FLAG_CEIL only", (unsigned)(flags & ~FQ_MX_FLAG_CEIL));
    if (rows < 0 || cols < 0) return fail(FQ_ERR_SHAPE, "negative shape rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (rows % 32 != 0) return fail(FQ_ERR_SHAPE, "rows=%lld is not a multiple of the 32-element MX block", (long long)rows);
    if (cols > 0 && rows > INT64_MAX / 4 / cols) return fail(FQ_ERR_SHAPE, "rows * cols overflows");
    if (rows == 0 || cols == 0) return ok();
    if (const int rc = mx_xy_pointers(x, y)) return rc;
    const int64_t row_bytes = cols * esize_of(dtype);
    if (row_bytes % 16 != 0) return fail(FQ_ERR_UNSUPPORTED, "cols=%lld: a row must be whole 16-byte vectors", (long long)cols);
    const int64_t ncs = row_bytes / 16, nct = (ncs + MXC_TILE_STRIPS - 1) / MXC_TILE_STRIPS;
    row_tiles = rows / MXC_TILE_ROWS;
    if (row_tiles > 0x7FFFFFFF / nct) return fail(FQ_ERR_UNSUPPORTED, "%lld x %lld tiles exceed one launch's grid", (long long)row_tiles, (long long)nct);
    a = MxColsArgs{x, y, ncs, (uint32_t)nct, rows * row_bytes >= NT_LOAD_MIN_BYTES ? 1 : 0};
    return CONTINUE;
}
MxSrKey sr_key(uint64_t seed, uint64_t stream_id) {
    return MxSrKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32)};
}
}  // namespace

// include/llmqat_fakequant_train.h
FQ_API int fqt_mx_fwd_cols(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, int flags, void* stream) {
    MxColsArgs a;
    int64_t row_tiles = 0;
    if (const int rc = mx_cols_checks(x, y, rows, cols, fmt, dtype, flags, a, row_tiles); rc != CONTINUE) return rc;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_mx_cols<decltype(dt)::value>((flags & FQ_MX_FLAG_CEIL) != 0, a, kMxFmts[fmt], row_tiles, st); });
}

// include/llmqat_fakequant_sr.h: the two forwards with stochastic rounding.  The checks are the nearest entry points' (mx_checks with the
// format and the flag bits first; mx_cols_checks), every one before any HIP call; any seed and stream id are valid.
FQ_API int fqs_mx_fwd(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, int flags, uint64_t seed, uint64_t stream_id,
                      void* stream) {
    auto first = [&] {
        if (fmt < FQ_MX_FP4_E2M1 || fmt > FQ_MX_FP8_E5M2) return fail(FQ_ERR_ARG, "unknown MX format code %d", fmt);
        if (flags & ~FQ_MX_FLAG_CEIL) return fail(FQ_ERR_ARG, "flag bits 0x%x: stochastic rounding takes FQ_MX_FLAG_CEIL only", (unsigned)(flags & ~FQ_MX_FLAG_CEIL));
        return 0;
    };
    int64_t nvec = 0;
    if (const int rc = mx_checks(dtype, rows, cols, false, nvec, first, [&] { return mx_xy_pointers(x, y); }); rc != CONTINUE) return rc;
    const MxArgs a{x, y, nullptr, nullptr, nvec, nvec * 16 >= NT_LOAD_MIN_BYTES ? 1 : 0};
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_mx_sr<decltype(dt)::value>((flags & FQ_MX_FLAG_CEIL) != 0, a, kMxFmts[fmt], sr_key(seed, stream_id), st); });
}

FQ_API int fqs_mx_fwd_cols(const void* x, void* y, int64_t rows, int64_t cols, int fmt, int dtype, int flags, uint64_t seed, uint64_t stream_id,
                           void* stream) {
    MxColsArgs a;
    int64_t row_tiles = 0;
    if (const int rc = mx_cols_checks(x, y, rows, cols, fmt, dtype, flags, a, row_tiles); rc != CONTINUE) return rc;
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) {
        return launch_mx_sr_cols<decltype(dt)::value>((flags & FQ_MX_FLAG_CEIL) != 0, a, kMxFmts[fmt], sr_key(seed, stream_id), row_tiles, st);
    });
}

// host only: no HIP call at all
FQ_API int fqs_mx_noise(uint64_t seed, uint64_t stream_id, int64_t first, int64_t n, int dtype, uint16_t* out) {
    if (dtype < 0 || dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", dtype);
    if (dtype == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the MX entry points");
    if (first < 0 || n < 0) return fail(FQ_ERR_SHAPE, "negative range first=%lld n=%lld", (long long)first, (long long)n);
    if (n > (int64_t)1 << 24) return fail(FQ_ERR_SHAPE, "n=%lld: at most 2^24 elements per call", (long long)n);
    if (first > INT64_MAX - n) return fail(FQ_ERR_SHAPE, "first + n overflows");
    if (n == 0) return ok();
    if (!out) return fail(FQ_ERR_NULL, "out must not be NULL");
    mx_sr_host_noise(sr_key(seed, stream_id), first, n, 16 / esize_of(dtype), out);
    return ok();
}

// Every check comes before any HIP call.
FQ_API int fq_mx_gemm(const void* a_elems, const void* a_scales, int a_fmt, const void* w_elems, const void* w_scales, int w_fmt, void* out,
                      int64_t M, int64_t N, int64_t K, int out_dtype, void* stream) {
    if (out_dtype < 0 || out_dtype > FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "unknown dtype code %d", out_dtype);
    if (out_dtype == FQ_DTYPE_F64) return fail(FQ_ERR_DTYPE, "float64 is not served by the MX entry points");
    for (int fmt : {a_fmt, w_fmt}) {
        if (fmt < FQ_MX_FP4_E2M1 || fmt > FQ_MX_FP8_E5M2) return fail(FQ_ERR_ARG, "unknown MX format code %d", fmt);
        if (fmt == FQ_MX_FP6_E2M3 || fmt == FQ_MX_FP6_E3M2) return fail(FQ_ERR_ARG, "FP6 formats have no export packing and no GEMM operand");
    }
    if (M < 0 || N < 0 || K < 0) return fail(FQ_ERR_SHAPE, "negative shape M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    if (M > 0x7FFFFFFF || N > 0x7FFFFFFF || K > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "M, N and K must be below 2^31 (byte offsets are 64-bit products of two)");
    if (K == 0 || K % MXG_KSTEP != 0) return fail(FQ_ERR_SHAPE, "K=%lld is not a positive multiple of %d", (long long)K, MXG_KSTEP);
    if (M == 0 || N == 0) return ok();
    if (!a_elems || !a_scales || !w_elems || !w_scales || !out) return fail(FQ_ERR_NULL, "a_elems / a_scales / w_elems / w_scales / out must not be NULL");
    if (!aligned16(a_elems) || !aligned16(w_elems) || !aligned16(out))
        return fail(FQ_ERR_UNSUPPORTED, "a_elems, w_elems and out must be 16-byte aligned");
    if (M > MXG_SKINNY_M && (N + MXG_TILE - 1) / MXG_TILE > 65535) return fail(FQ_ERR_UNSUPPORTED, "N=%lld exceeds one launch's grid", (long long)N);
    const MxGemmArgs g{(const uint8_t*)w_elems, (const uint8_t*)w_scales, (const uint8_t*)a_elems, (const uint8_t*)a_scales, out, M, N, K, w_fmt, a_fmt, out_dtype};
    return launch_mx_gemm(g, (hipStream_t)stream);
}

// include/llmqat_fakequant_infer.h: an export back to a tensor.  mx_checks' list with the export's format refusals first (the FP6 one in
// fq_mx_export's words); nvec counts the OUTPUT's vectors.  Every check comes before any HIP call.
FQ_API int fqi_mx_dequant(const void* elems, const void* scales, void* y, int64_t rows, int64_t cols, int fmt, int dtype, void* stream) {
    auto formats = [&] {
        if (fmt < FQ_MX_FP4_E2M1 || fmt > FQ_MX_FP8_E5M2) return fail(FQ_ERR_ARG, "unknown MX format code %d", fmt);
        if (fmt == FQ_MX_FP6_E2M3 || fmt == FQ_MX_FP6_E3M2) return fail(FQ_ERR_ARG, "FP6 formats have no export packing");
        return 0;
    };
    auto pointers = [&] {
        if (!elems || !scales || !y) return fail(FQ_ERR_NULL, "elems / scales / y must not be NULL");
        if (!aligned16(elems) || !aligned16(y)) return fail(FQ_ERR_UNSUPPORTED, "elems and y must be 16-byte aligned");
        return 0;
    };
    int64_t nvec = 0;
    if (const int rc = mx_checks(dtype, rows, cols, false, nvec, formats, pointers); rc != CONTINUE) return rc;
    const MxDequantArgs a{(const uint8_t*)elems, (const uint8_t*)scales, y, nvec};
    hipStream_t st = (hipStream_t)stream;
    return by_dtype(dtype, [&](auto dt) { return launch_mx_dequant<decltype(dt)::value>(fmt, a, st); });
}

}  // extern "C"
