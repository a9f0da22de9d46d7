// fq_dtype_impl.h -- kernel selection + launches for ONE element type (included by fq_<dtype>.hip).
#pragma once
#include "../../include/llmqat_fakequant.h"
#include "fq_launch.h"


namespace fq {

// Which (threads per row, 16-byte vectors per thread) the model widths select (bf16 / fp16: 8 elements per vector):
//   4096 -> 512 vectors -> 256 x 2     5120 -> 640 -> 256 x 3     11008 -> 1376 -> 512 x 3     13824 -> 1728 -> 512 x 4
//   tiny-LLaMA (fp32, 4 per vector): 256 -> 64 x 1, 688 -> 64 x 3.      Every other width is served by the nearest shape that holds it.
// Round 4 pruned the instantiations nothing selects often enough to deserve its own code (27 MB / 100 s of build in round 3): stores
// are always non-temporal (two cache-policy flavours instead of three; round 6: `nt sc1` on the streamed Sym forward and the two-slot
// mask backward, below), 5 / 7 vectors per thread share the 6 / 8 kernels.
// Launch shape of the register-resident kernel, from tools/kbench on MI355X: 2-3 vectors per
// thread is the sweet spot (round 3 re-checked with block sizes that are not powers of two -- 704 x 2 for 11008 cols wastes 2 % of
// the vector slots instead of 10 %, 576 x 3 for 13824, 320 x 2 for 5120 -- and with 256 x 6 for mid-sized tensors: within +-2 % of
// the shapes below everywhere, profiles/r03_kbench_block_shapes.txt, r03_ab_mid_rows_256.txt) (11008 bf16 cols: 512 thr x 3 = 30.6 us, 256 x 6 = 31.1, 1024 x 2 = 32.2;
// 4096 cols: 256 x 2 = 6.1 us, 128 x 4 = 6.3, 64 x 8 = 6.9, 512 x 1 = 7.7).
// The ladder itself is by_reg_shape (fq_shapes.h); the plain and the autocast (AC = 1) forward both launch through here.
template <int DT, bool ASYM, bool FAST, bool NTL, int NTS, bool DBG, int AC = 0, bool PITCH = false>
static void launch_reg(const RowArgs& a, int64_t nvec, hipStream_t st) {
    by_reg_shape(nvec, [&](auto tpr, auto vpt) {
        constexpr int TPR = decltype(tpr)::value, VPT = decltype(vpt)::value;
        launch_rows<TPR>(row_reg_kernel<DT, TPR, VPT, ASYM, FAST, NTL, NTS, DBG, AC, PITCH>, a.rows, st, a);
    });
}

template <int DT, int TPR, bool NTL, bool NTS, bool PITCH = false>
static void launch_wide(const RowArgs& a, int hpt, hipStream_t st) {
    const bool mask = any_mask(a) || PITCH;  // the mask-recording code lives in its own instantiation (it costs the plain one 7 %); pitched rows: one flavour
    by_count(hpt, [&](auto n) {
        constexpr int HPT = decltype(n)::value == 7 ? 8 : decltype(n)::value;   // 7 half-vectors per thread run as 8
        if (mask) launch_rows<TPR>(row_reg_wide_kernel<DT, TPR, HPT, NTL, NTS, true, PITCH>, a.rows, st, a);
        else if constexpr (!PITCH) launch_rows<TPR>(row_reg_wide_kernel<DT, TPR, HPT, NTL, NTS, false>, a.rows, st, a);
    });
}

// the scalar-load kernel (any width up to GENERIC_MAX_COLS, any alignment): one wave per row up to 1024 columns, a 256-thread block beyond
template <int DT, bool ASYM, int AC = 0> static void launch_generic(const RowArgs& a, hipStream_t st) {
    if (a.cols <= 1024) launch_rows<64>(row_generic_kernel<DT, 64, ASYM, AC>, a.rows, st, a);
    else launch_rows<256>(row_generic_kernel<DT, 256, ASYM, AC>, a.rows, st, a);
}

// Very long rows (layerwise): two passes -- the row statistics through atomics into the workspace (vec: in 16-byte vectors), then
// `apply`, which takes a row in chunks of `ach` elements.  Every refusal comes before the workspace is touched.
template <int DT, bool ASYM>
static int two_pass(const RowArgs& a, bool vec, void (*apply)(RowArgs, const uint32_t*, int64_t), int64_t ach, void* ws, size_t wsb, hipStream_t st) {
    if (any_pitch(a)) return fail(FQ_ERR_UNSUPPORTED, "rows that do not follow one another: not served by the two-pass path");
    if (!ws || wsb < (size_t)a.rows * 8)
        return fail(FQ_ERR_WORKSPACE, "two-pass path needs %zu workspace bytes, got %zu", (size_t)a.rows * 8, wsb);
    const int64_t sch = vec ? tp_chunk_elems<DT, true>() : tp_chunk_elems<DT, false>();
    const int64_t schunks = (a.cols + sch - 1) / sch, achunks = (a.cols + ach - 1) / ach;
    if (a.rows * schunks > 0x7FFFFFFF || a.rows * achunks > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows*chunks exceeds the grid limit");
    if (hipMemsetAsync(ws, 0, (size_t)a.rows * 8, st) != hipSuccess) return fail(FQ_ERR_LAUNCH, "hipMemsetAsync failed");
    uint32_t* w = (uint32_t*)ws;
    if (vec) launch_grid(stats_kernel<DT, ASYM, true>, a.rows * schunks, 1, TP_THREADS, st, a, w, schunks);
    else launch_grid(stats_kernel<DT, ASYM, false>, a.rows * schunks, 1, TP_THREADS, st, a, w, schunks);
    launch_grid(apply, a.rows * achunks, 1, TP_THREADS, st, a, (const uint32_t*)w, achunks);
    return launch_result();
}

template <int DT, int AC>
static int sym_autocast_t(RowArgs a, void* ws, size_t wsb, hipStream_t st) {
    using T = Ty<DT>;
    begin_launches();
    seal_slots(a);
    if constexpr (T::ESIZE != 2) {
        return fail(FQ_ERR_DTYPE, "autocast arithmetic applies to bf16 / fp16 tensors only");
    } else {
        constexpr int EPV = 8;
        const bool pair = a.n_more > 0;
        const bool vec_ok = aligned16(a.x) && aligned16(a.y) && (a.cols % EPV == 0) && more_aligned(a, 15u, 15u) && pitches_aligned(a, 15, 15);
        const int64_t nvec = a.cols / EPV;
        const int64_t big_rows = largest_rows(a);
        const int64_t bytes = big_rows * a.cols * T::ESIZE;
        if (a.rows > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows=%lld exceeds the grid limit", (long long)a.rows);
        const bool pitched = any_pitch(a);
        if constexpr (AC == 2) {
            // fp32 result: 8-byte loads / 16-byte stores keep both streams fully coalesced
            const int64_t nh = a.cols / 4;
            const bool wide_ok = aligned16(a.y) && (reinterpret_cast<uintptr_t>(a.x) & 7u) == 0 && a.cols % 4 == 0 && nh <= 1024 * 8 &&
                                 more_aligned(a, 7u, 15u) && pitches_aligned(a, 7, 15);
            if (wide_ok) {
                const bool ntl = bytes >= NT_LOAD_MIN_BYTES;
                auto wide = [&](auto tpr) {
                    constexpr int TPR = decltype(tpr)::value;
                    const int hpt = (int)((nh + TPR - 1) / TPR);
                    if (pitched) launch_wide<DT, TPR, false, true, true>(a, hpt, st);
                    else if (ntl) launch_wide<DT, TPR, true, true>(a, hpt, st);
                    else launch_wide<DT, TPR, false, true>(a, hpt, st);
                };
                if (nh <= 512) wide(Const<64>{});
                else if (nh <= 2048) wide(Const<256>{});
                else wide(Const<1024>{});
                return launch_result();
            }
            if (pair || a.mask)
                return fail(FQ_ERR_UNSUPPORTED, "fp32-result forward with STE mask / second tensor: rows must be 8-byte aligned, cols %% 4 == 0, cols <= 32768");
            // other shapes: scalar-load kernel or two passes (bounds only)
            if (a.cols <= GENERIC_MAX_COLS) {
                launch_generic<DT, false, AC>(a, st);
                return launch_result();
            }
        } else {
            if (pair && !(vec_ok && nvec <= REG_MAX_VEC))
                return fail(FQ_ERR_UNSUPPORTED, "pair launch: rows must be 16-byte aligned and fit the register kernels");
        }
        if (AC == 1 && vec_ok && nvec <= REG_MAX_VEC) {
            if constexpr (AC == 1) {
                if (pitched) launch_reg<DT, false, false, false, ST_NT, false, AC, true>(a, nvec, st);   // rows that do not follow one another: their own instantiations
                else if (bytes >= NT_LOAD_MIN_BYTES) launch_reg<DT, false, false, true, ST_NT, false, AC>(a, nvec, st);
                else launch_reg<DT, false, false, false, ST_NT, false, AC>(a, nvec, st);
            }
        } else if (a.mask) {
            return fail(FQ_ERR_UNSUPPORTED, "STE-mask forward needs 16-byte aligned rows that fit the register kernels");
        } else if (a.cols <= GENERIC_MAX_COLS) {
            launch_generic<DT, false, AC>(a, st);
        } else {  // very long rows (layerwise): |x| max per row through atomics, then apply in element loads
            return two_pass<DT, false>(a, aligned16(a.x) && a.cols % EPV == 0, apply_autocast_kernel<DT, AC == 2>, TP_THREADS * TP_EPT, ws, wsb, st);
        }
        return launch_result();
    }
}

template <int DT> int launch_sym_autocast(bool wide, RowArgs a, void* ws, size_t wsb, hipStream_t st) {
    return wide ? sym_autocast_t<DT, 2>(a, ws, wsb, st) : sym_autocast_t<DT, 1>(a, ws, wsb, st);
}

template <int DT, bool ASYM, bool FAST>
static int rowwise_t(RowArgs a, void* ws, size_t wsb, hipStream_t st) {
    using T = Ty<DT>;
    begin_launches();
    seal_slots(a);
    constexpr int EPV = 16 / T::ESIZE;
    const bool pair = a.n_more > 0;  // several tensors in one launch: register kernels only
    const bool vec_ok = aligned16(a.x) && aligned16(a.y) && (a.cols % EPV == 0) && more_aligned(a, 15u, 15u) && pitches_aligned(a, 15, 15);
    const int64_t nvec = a.cols / EPV;
    const int64_t big_rows = largest_rows(a);
    const int64_t bytes = big_rows * a.cols * T::ESIZE;  // cache policy follows the larger tensor
    const bool pitched = any_pitch(a);
    const bool ntl = bytes >= NT_LOAD_MIN_BYTES;
    if (pair && !(vec_ok && nvec <= REG_MAX_VEC)) return fail(FQ_ERR_UNSUPPORTED, "pair launch: rows must be 16-byte aligned and fit the register kernels");
    if (vec_ok && nvec <= REG_MAX_VEC) {
        if (a.rows > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows=%lld exceeds the grid limit", (long long)a.rows);
        // the diagnostic outputs (bin indices, scales) live in their own instantiation so the product
        // kernels carry none of that code; it runs the same arithmetic with the default cache policy
        if (a.idx || a.scale) launch_reg<DT, ASYM, FAST, false, false, true>(a, nvec, st);
        else if (pitched) launch_reg<DT, ASYM, FAST, false, true, false, 0, true>(a, nvec, st);   // rows that do not follow one another: their own instantiations
        // streamed Sym tensors (the pair forward): y stores nt sc1, 2.5 % faster than nt on the W4 + A8 [4096, 11008] pair
        // (59.6 -> 58.1 us, tools/fwd_variants.hip, profiles/r06_ab_store_policy.txt); Asym keeps nt (not measured)
        else if (ntl) launch_reg<DT, ASYM, FAST, true, ASYM ? ST_NT : ST_NT_SC1, false>(a, nvec, st);
        else launch_reg<DT, ASYM, FAST, false, true, false>(a, nvec, st);
    } else if (a.mask) {
        return fail(FQ_ERR_UNSUPPORTED, "STE-mask forward needs 16-byte aligned rows that fit the register kernels");
    } else if (vec_ok && !pitched) {
        return two_pass<DT, ASYM>(a, true, apply_kernel<DT, ASYM, FAST, true>, tp_chunk_elems<DT, true>(), ws, wsb, st);
    } else if (a.cols <= GENERIC_MAX_COLS) {
        if (a.rows > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows=%lld exceeds the grid limit", (long long)a.rows);
        launch_generic<DT, ASYM>(a, st);
    } else {
        return two_pass<DT, ASYM>(a, false, apply_kernel<DT, ASYM, FAST, false>, tp_chunk_elems<DT, false>(), ws, wsb, st);
    }
    return launch_result();
}

template <int DT> int launch_rowwise(bool asym, bool fast, RowArgs a, void* ws, size_t wsb, hipStream_t st) {
    if constexpr (DT == BF16) {
        // bf16, <= 8 bits: the IEEE divides become multiplies with a reciprocal -- provably
        // bit-identical after the bf16 rounding (DESIGN.md "Numerics").
        if (fast) return asym ? rowwise_t<DT, true, true>(a, ws, wsb, st) : rowwise_t<DT, false, true>(a, ws, wsb, st);
    }
    if constexpr (DT == F16) {
        // fp16 AsymQuantizer at <= 8 bits: FAST selects the lookup-table form of the register kernel (exact arithmetic kept)
        if (fast && asym) return rowwise_t<DT, true, true>(a, ws, wsb, st);
    }
    return asym ? rowwise_t<DT, true, false>(a, ws, wsb, st) : rowwise_t<DT, false, false>(a, ws, wsb, st);
}

template <int DT> int launch_ste(const void* g, const void* x, void* gx, int64_t n, float lo, float hi, hipStream_t st) {
    using T = Ty<DT>;
    begin_launches();
    constexpr int EPV = 16 / T::ESIZE;
    if (aligned16(g) && aligned16(x) && aligned16(gx) && n % EPV == 0) {
        const int64_t nvec = n / EPV;
        const int64_t grid = (nvec + STE_THREADS - 1) / STE_THREADS;  // one vector per thread measured best (kbench)
        if (grid > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "n too large");
        const int64_t bytes = n * T::ESIZE;
        if (bytes >= NT_LOAD_MIN_BYTES)
            launch_grid(ste_vec_kernel<DT, 1, true, true>, grid, 1, STE_THREADS, st, (const uint4*)g, (const uint4*)x, (uint4*)gx, nvec, lo, hi);
        else
            launch_grid(ste_vec_kernel<DT, 1, false, true>, grid, 1, STE_THREADS, st, (const uint4*)g, (const uint4*)x, (uint4*)gx, nvec, lo, hi);
    } else {
        int64_t grid = (n + STE_THREADS - 1) / STE_THREADS;
        if (grid > 8192) grid = 8192;
        launch_grid(ste_scalar_kernel<DT>, grid, 1, STE_THREADS, st, g, x, gx, n, lo, hi);
    }
    return launch_result();
}

template <int DT>
int launch_ste_rows(const void* g, const void* x, void* gx, int64_t rows, int64_t cols, float lo, float hi, const float* bounds,
                    hipStream_t st, const StePitch3& pitch) {
    using T = Ty<DT>;
    begin_launches();
    constexpr int EPV = 16 / T::ESIZE;
    const bool pitched = pitch.g.on || pitch.x.on || pitch.o.on;
    if (!(aligned16(g) && aligned16(x) && aligned16(gx) && cols % EPV == 0 && pitch_aligned(pitch.g, 15) && pitch_aligned(pitch.x, 15) && pitch_aligned(pitch.o, 15))) {
        if (pitched) return fail(FQ_ERR_UNSUPPORTED, "rows that do not follow one another: the STE backward needs 16-byte aligned rows of whole vectors");
        return launch_ste<DT>(g, x, gx, rows * cols, lo, hi, st);  // odd layout: plain path, same result
    }
    if (pitched && rows > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows exceed the grid limit");
    const int64_t nvec_row = cols / EPV;
    // balanced chunks: every block of a row gets the same number of vectors (<= 256 x 8)
    const int64_t chunks = (nvec_row + STE_THREADS * 8 - 1) / (STE_THREADS * 8);
    const int cv = (int)((nvec_row + chunks - 1) / chunks);
    const int vpt = (cv + STE_THREADS - 1) / STE_THREADS;
    if (rows * chunks > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows*chunks exceeds the grid limit");
    const int64_t bytes = rows * cols * T::ESIZE;
    const bool ntl = bytes >= NT_LOAD_MIN_BYTES;
    by_count(vpt, [&](auto n) {
        constexpr int V = decltype(n)::value;
        auto go = [&](auto kern) { launch_grid(kern, rows * chunks, 1, STE_THREADS, st, g, x, gx, nvec_row, chunks, cv, bounds, lo, hi, pitch); };
        if (pitched) go(ste_rows_kernel<DT, V, false, true, true>);
        else if (ntl) go(ste_rows_kernel<DT, V, true, true>);
        else go(ste_rows_kernel<DT, V, false, true>);
    });
    return launch_result();
}

// block layout of a mask-backward launch (grid x): copying slots get one block per row, in-place slots one per STE_THREADS rows;
// grid y = chunks of a row.  Unused slots: blk_begin = INT64_MAX (ste_pick_slot compares against all four).
inline int64_t ste_layout(SteLaunch& L, bool allow_inplace) {
    int64_t blk = 0;
    for (int i = 0; i < 1 + MAX_MORE; ++i) {
        if (i >= L.n) {
            L.t[i] = SteSlot{};
            L.t[i].blk_begin = INT64_MAX;
            continue;
        }
        L.t[i].blk_begin = blk;
        L.t[i].inplace = allow_inplace && L.t[i].gx == (const void*)L.t[i].g;
        blk += L.t[i].inplace ? (L.t[i].rows + STE_THREADS - 1) / STE_THREADS : L.t[i].rows;
    }
    return blk;
}

template <int DT> int launch_ste_mask(SteLaunch L, int64_t cols, float lo, float hi, hipStream_t st) {
    using T = Ty<DT>;
    begin_launches();
    constexpr int EPV = 16 / T::ESIZE;
    const int64_t mrw = mask_row_words(cols, T::ESIZE);
    if (!mrw) return fail(FQ_ERR_UNSUPPORTED, "STE-mask backward: shape not served");
    for (int i = 0; i < L.n; ++i)
        if (!(aligned16(L.t[i].g) && aligned16(L.t[i].gx) && (reinterpret_cast<uintptr_t>(L.t[i].mask) & 7u) == 0 && pitch_aligned(L.t[i].gp, 15) &&
              pitch_aligned(L.t[i].op, 15)))
            return fail(FQ_ERR_UNSUPPORTED, "STE-mask backward: alignment not served (g / gx rows 16 bytes, mask 8 bytes)");
    const int64_t nvec_row = cols / EPV;
    const int64_t chunks = (nvec_row + STE_THREADS * 8 - 1) / (STE_THREADS * 8);
    int cv = (int)((nvec_row + chunks - 1) / chunks);
    cv = (cv + 63) / 64 * 64;  // whole waves per slot
    const int vpt = (cv + STE_THREADS - 1) / STE_THREADS;
    const int64_t grid = ste_layout(L, true);
    if (grid > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows exceed the grid limit");
    int64_t big_rows = 0;  // cache policy follows the largest tensor that is actually streamed
    for (int i = 0; i < L.n; ++i)
        if (!L.t[i].inplace && L.t[i].rows > big_rows) big_rows = L.t[i].rows;
    const int64_t bytes = big_rows * cols * T::ESIZE;
    const bool ntl = bytes >= NT_LOAD_MIN_BYTES;
    bool pitched = false;
    for (int i = 0; i < L.n; ++i) pitched = pitched || L.t[i].gp.on || L.t[i].op.on;
    by_count(vpt, [&](auto n) {
        constexpr int V = decltype(n)::value;
        auto go = [&](auto kern) { launch_grid(kern, grid, chunks, STE_THREADS, st, L, nvec_row, cv, mrw, lo, hi); };
        if (L.n == 1 && !L.t[0].inplace && !pitched) {   // one copying tensor: its own lean kernel (fq_kernels.h, ste_mask_one_kernel)
            const SteSlot& t0 = L.t[0];
            auto one = [&](auto kern) { launch_grid(kern, grid, chunks, STE_THREADS, st, t0.g, t0.gx, t0.bounds, t0.mask, nvec_row, cv, mrw, lo, hi); };
            if (ntl) one(ste_mask_one_kernel<DT, V, true, true>);
            else one(ste_mask_one_kernel<DT, V, false, true>);
        } else if (L.n <= 2 && !pitched) {
            // two tensors (a QuantizeLinear's weight + input): the slot pick looks at two slots instead of four.  Streamed gx stores nt sc1: the
            // W4 + A8 [4096, 11008] forward + backward pair 2.0 % faster with both launches' stores nt sc1 (profiles/r06_ab_store_policy.txt)
            if (ntl) go(ste_mask_kernel<DT, V, true, ST_NT_SC1, false, 2>);
            else go(ste_mask_kernel<DT, V, false, true, false, 2>);
        } else if (pitched) go(ste_mask_kernel<DT, V, false, true, true>);
        else if (ntl) go(ste_mask_kernel<DT, V, true, true>);
        else go(ste_mask_kernel<DT, V, false, true>);
    });
    return launch_result();
}

template <int DT> int launch_ste_mask_wide(SteLaunch L, int64_t cols, float lo, float hi, hipStream_t st) {
    using T = Ty<DT>;
    begin_launches();
    if constexpr (T::ESIZE != 2) {
        return fail(FQ_ERR_DTYPE, "fp32-gradient STE backward applies to bf16 / fp16 inputs only");
    } else {
        const int64_t mrw = mask_row_words(cols, T::ESIZE);
        auto al8 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; };
        if (!mrw || cols > 32768) return fail(FQ_ERR_UNSUPPORTED, "fp32-gradient STE backward: shape not served");
        for (int i = 0; i < L.n; ++i)
            if (!(aligned16(L.t[i].g) && al8(L.t[i].gx) && al8(L.t[i].mask) && pitch_aligned(L.t[i].gp, 15) && pitch_aligned(L.t[i].op, 7)))
                return fail(FQ_ERR_UNSUPPORTED, "fp32-gradient STE backward: alignment not served");
        const int64_t nh_row = cols / 4;
        const int64_t chunks = (nh_row + STE_THREADS * 8 - 1) / (STE_THREADS * 8);
        int ch = (int)((nh_row + chunks - 1) / chunks);
        ch = (ch + 63) / 64 * 64;
        const int hpt = (ch + STE_THREADS - 1) / STE_THREADS;
        const int64_t grid = ste_layout(L, false);
        if (grid > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows exceed the grid limit");
        const int64_t bytes = largest_rows(L) * cols * 4;  // the fp32 gradient is the larger stream
        const bool ntl = bytes >= NT_LOAD_MIN_BYTES;
        bool pitched = false;
        for (int i = 0; i < L.n; ++i) pitched = pitched || L.t[i].gp.on || L.t[i].op.on;
        by_count(hpt, [&](auto n) {
            constexpr int V = decltype(n)::value;
            auto go = [&](auto kern) { launch_grid(kern, grid, chunks, STE_THREADS, st, L, nh_row, ch, mrw, lo, hi); };
            if (!ntl && !pitched && L.n <= 2) {   // the K / V-sized launches: one or two slots instead of a four-slot pick in every block's prologue
                if (L.n == 1) go(ste_mask_wide_kernel<DT, V, false, true, false, 1>);
                else go(ste_mask_wide_kernel<DT, V, false, true, false, 2>);
            } else if (pitched) go(ste_mask_wide_kernel<DT, V, false, true, true>);
            else if (ntl) go(ste_mask_wide_kernel<DT, V, true, true>);
            else go(ste_mask_wide_kernel<DT, V, false, true>);
        });
        return launch_result();
    }
}

template <int DT>
int launch_w12(const void* w, const void* scale, void* out, int64_t rows, int64_t cols, int w_bits, int scale_per_row, float cv,
               hipStream_t st) {
    using T = Ty<DT>;
    begin_launches();
    constexpr int EPV = 16 / T::ESIZE;
    const bool vec = aligned16(w) && aligned16(out) && cols % EPV == 0;
    int64_t grid = vec ? (rows * (cols / EPV) + 255) / 256 : (rows * cols + 255) / 256;
    if (!vec && grid > 16384) grid = 16384;
    if (grid > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "tensor too large");
    if (w_bits == 1) {
        if (vec) launch_grid(w12_kernel<DT, 1, true>, grid, 1, 256, st, w, scale, out, rows, cols, scale_per_row, cv);
        else launch_grid(w12_kernel<DT, 1, false>, grid, 1, 256, st, w, scale, out, rows, cols, scale_per_row, cv);
    } else {
        if (vec) launch_grid(w12_kernel<DT, 2, true>, grid, 1, 256, st, w, scale, out, rows, cols, scale_per_row, cv);
        else launch_grid(w12_kernel<DT, 2, false>, grid, 1, 256, st, w, scale, out, rows, cols, scale_per_row, cv);
    }
    return launch_result();
}

// The one-launch 1-/2-bit branch with ATen's own summation order (w12_row_aten_kernel): served where that order is the restated one --
// contiguous rows >= 8, cols >= 256, cols % 4 == 0, 16-byte aligned tensors, rows that fit the kernel's registers.
template <int DT>
int launch_w12_rows(const void* w, void* out, void* scale_out, int64_t rows, int64_t cols, int w_bits, float cv, hipStream_t st) {
    using T = Ty<DT>;
    if (!(aligned16(w) && aligned16(out) && cols % 4 == 0 && cols >= 256 && rows >= 8))
        return fail(FQ_ERR_UNSUPPORTED, "one-launch 1-/2-bit branch: needs rows >= 8, cols >= 256, cols %% 4 == 0 and 16-byte aligned tensors");
    if (rows > 0x7FFFFFFF) return fail(FQ_ERR_SHAPE, "rows=%lld exceeds the grid limit", (long long)rows);
    const int64_t ngroups = cols / 4;
    const bool shared_row = cols >= 8129;                      // ATen: values_per_thread = ceil(cols / 64) >= 128 splits a row across the 8 waves
    const int64_t gpt = shared_row ? (ngroups + 511) / 512 : (ngroups + 63) / 64;   // groups per ATen thread
    constexpr int MAXG_OWN = DT == F32 ? 16 : 32;              // fp32 groups are 4 VGPRs each
    if (gpt > (shared_row ? 16 : MAXG_OWN) || (shared_row && (cols + 511) / 512 >= 256))
        return fail(FQ_ERR_UNSUPPORTED, "one-launch 1-/2-bit branch: cols=%lld outside the row lengths this kernel holds in registers", (long long)cols);
    begin_launches();
    const float factor = (float)rows / (float)(rows * cols);   // ATen: static_cast<float>(num_outputs) / numel
    const bool ntl = rows * cols * T::ESIZE >= NT_LOAD_MIN_BYTES;
    const int64_t grid = shared_row ? rows : (rows + 7) / 8;
    auto go = [&](auto sh, auto g) {   // sh: a row is shared by the 8 waves; g: groups of 4 elements a thread holds
        constexpr bool SH = decltype(sh)::value;
        constexpr int G = decltype(g)::value;
        auto bits = [&](auto wb) {
            constexpr int WB = decltype(wb)::value;
            if (ntl) launch_grid(w12_row_aten_kernel<DT, WB, SH, G, true, true>, grid, 1, 512, st, w, out, scale_out, rows, cols, cv, factor);
            else launch_grid(w12_row_aten_kernel<DT, WB, SH, G, false, true>, grid, 1, 512, st, w, out, scale_out, rows, cols, cv, factor);
        };
        if (w_bits == 1) bits(Const<1>{});
        else bits(Const<2>{});
    };
    if (shared_row) {
        if (gpt <= 6) go(std::true_type{}, Const<6>{});
        else if (gpt <= 8) go(std::true_type{}, Const<8>{});
        else go(std::true_type{}, Const<16>{});
    } else {
        if (gpt <= 16) go(std::false_type{}, Const<16>{});
        else if constexpr (DT != F32) go(std::false_type{}, Const<32>{});
    }
    return launch_result();
}

#define FQ_INSTANTIATE(DT)                                                                                      \
    template int launch_rowwise<DT>(bool, bool, RowArgs, void*, size_t, hipStream_t);                           \
    template int launch_sym_autocast<DT>(bool, RowArgs, void*, size_t, hipStream_t);                                           \
    template int launch_ste<DT>(const void*, const void*, void*, int64_t, float, float, hipStream_t);           \
    template int launch_ste_rows<DT>(const void*, const void*, void*, int64_t, int64_t, float, float, const float*, hipStream_t, const StePitch3&); \
    template int launch_ste_mask<DT>(SteLaunch, int64_t, float, float, hipStream_t);                             \
    template int launch_ste_mask_wide<DT>(SteLaunch, int64_t, float, float, hipStream_t);                        \
    template int launch_w12<DT>(const void*, const void*, void*, int64_t, int64_t, int, int, float, hipStream_t);     \
    template int launch_w12_rows<DT>(const void*, void*, void*, int64_t, int64_t, int, float, hipStream_t);

}  // namespace fq
