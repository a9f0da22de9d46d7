// fq_group.h -- group-wise fake quantization: every run of `g` consecutive elements of a row has its own scale.
//
//   group_reg_kernel    the register-resident layout of row_reg_kernel (thread t owns 16-byte vectors t + i*TPR, TPR a multiple of
//                       64), with the reduction done per GROUP: a group is GV = g * esize / 16 vectors, and because TPR is a multiple
//                       of GV, slot i of an aligned GV-lane segment holds exactly one group.  The group max (Sym) or min/max (Asym)
//                       is therefore a sub-wave reduction (DPP inside a 16-lane row, one ds_swizzle across rows for GV = 32, two
//                       v_readlane for GV = 64): no LDS, no barrier.  Each lane then derives its slot's scale with the row-wise
//                       scalar code (sym_row / sym_row_autocast / asym_row) and runs the row-wise element chains.
//                       Training mode writes the side outputs of the FULL row, in the layout fq_*_fwd_train writes them (row
//                       bounds = the row's max / min from one block reduction of the lane extremes, the ABI-3 bitmap), so the
//                       existing mask backwards serve it unchanged.  Plain mode needs no block reduction at all.
// Semantics: y = Q(x.reshape(-1, g)).reshape(x.shape) with Q the row-wise quantizer of the same arithmetic; every NaN / Inf / +-0 rule
// applies per group (a NaN poisons its own group only).
#pragma once
#include "fq_launch.h"

namespace fq {

// idempotent reduction over aligned groups of gv lanes (gv in {4, 8, 16, 32, 64}, block-uniform); all 64 lanes active
template <class Op> __device__ __forceinline__ uint32_t group_reduce(uint32_t v, int gv) {
    v = Op::f(v, dpp<0xB1>(v));                       // quad_perm:[1,0,3,2]
    v = Op::f(v, dpp<0x4E>(v));                       // quad_perm:[2,3,0,1]   -> quads uniform
    if (gv >= 8) v = Op::f(v, dpp<0x141>(v));         // row_half_mirror        -> 8 lanes
    if (gv >= 16) v = Op::f(v, dpp<0x140>(v));        // row_mirror             -> 16 lanes
    if (gv >= 32) v = Op::f(v, (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F));   // bit mode, xor 16 -> 32 lanes
    if (gv >= 64) v = Op::f((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 32));
    return v;
}

struct GroupArgs {
    int gv;    // vectors per group
    int ntl;   // non-temporal loads (the tensor is larger than NT_LOAD_MIN_BYTES): a block-uniform branch, not an instantiation
};

template <int DT, int TPR, int VPT, bool ASYM, bool FAST, int AC>
__global__ __launch_bounds__(TPR == 64 ? 256 : TPR) void group_reg_kernel(RowArgs a, GroupArgs ga) {
    using T = Ty<DT>;
    static_assert(AC == 0 || (AC == 1 && !ASYM && T::ESIZE == 2), "autocast arithmetic: Sym on 16-bit tensors");
    static_assert(TPR % 64 == 0, "a group must never straddle two waves");
    constexpr int EPV = 16 / T::ESIZE;
    constexpr int NW = TPR / 64;
    constexpr bool AFAST = FAST && DT == BF16;
    __shared__ uint32_t red[3][NW > 1 ? NW : 1];

    int64_t row;
    int t;
    if (!row_and_lane<TPR>(a.rows, row, t)) return;
    const int nvec = (int)(a.cols / EPV);
    const uint4* __restrict__ xr = (const uint4*)((const char*)a.x + row * a.cols * T::ESIZE);
    uint4* __restrict__ yr = (uint4*)((char*)a.y + row * a.cols * T::ESIZE);

    // Out-of-range slots re-load the row's last vector.  nvec is a multiple of GV and segments are GV-aligned, so such a slot's whole
    // segment is out of range: its (duplicate) values only ever meet the row bounds, where max / min are idempotent.
    uint4 r[VPT];  // (load_clamped() written out: through the helper the VPT == 1 instantiations swap the two arms of this branch)
    if (ga.ntl) {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int v = t + i * TPR;
            r[i] = ld16<true>(&xr[v < nvec ? v : nvec - 1]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            const int v = t + i * TPR;
            r[i] = ld16<false>(&xr[v < nvec ? v : nvec - 1]);
        }
    }

    const bool want_bounds = a.bounds != nullptr;   // training mode (a mask always comes with bounds): uniform over the launch
    SymRow sr[ASYM ? 1 : VPT];
    AsymRow ar[ASYM ? VPT : 1];
    float ub = 0.f, lb = 0.f;  // bounds of the row's values (training mode only)
    if constexpr (!ASYM) {
        uint32_t lane_m = 0;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            uint32_t acc = 0;
            acc = T::absmax_acc(acc, r[i].x);
            acc = T::absmax_acc(acc, r[i].y);
            acc = T::absmax_acc(acc, r[i].z);
            acc = T::absmax_acc(acc, r[i].w);
            const uint32_t mbits = group_reduce<OpMaxU>(T::absmax_finish(acc), ga.gv);
            lane_m = lane_m > mbits ? lane_m : mbits;
            if constexpr (AC == 0) sr[i] = sym_row<DT>(as_f(mbits), a.sym);
            else sr[i] = sym_row_autocast<DT>(as_f(mbits), a.sym);
        }
        if (want_bounds) {
            const float m = as_f(block_reduce<OpMaxU, NW>(lane_m, red[0]));
            ub = m;
            lb = -m;
            if (t == 0) store_bounds(a.bounds, row, m, -m);
        }
    } else if constexpr (T::ESIZE == 2) {  // min and max on the raw bits (order-preserving 16-bit keys), as row_reg_kernel
        uint32_t lane_w = 0;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            MinMaxKeys mk;
            mk.acc(r[i].x);
            mk.acc(r[i].y);
            mk.acc(r[i].z);
            mk.acc(r[i].w);
            const uint32_t w = group_reduce<OpPkMaxU16>(mk.word(), ga.gv);
            lane_w = OpPkMaxU16::f(lane_w, w);
            float mx, mn;
            minmax_from_keys<DT>(w, mx, mn);
            ar[i] = asym_row<DT>(mx, mn, a.asym);
        }
        if (want_bounds) {
            minmax_from_keys<DT>(block_reduce<OpPkMaxU16, NW>(lane_w, red[0]), ub, lb);
            if (t == 0) store_bounds(a.bounds, row, ub, lb);
        }
    } else {  // fp32: v_max_f32 / v_min_f32 with NaN tracked through the |x| bits, as row_reg_kernel
        uint32_t lane_nb = 0, lane_mx = 0, lane_mn = 0;
#pragma unroll
        for (int i = 0; i < VPT; ++i) {
            MinMax mm;
            mm.mx = mm.mn = as_f(r[i].x);
            mm.absacc = 0;
            minmax_acc<DT>(mm, r[i].x);
            minmax_acc<DT>(mm, r[i].y);
            minmax_acc<DT>(mm, r[i].z);
            minmax_acc<DT>(mm, r[i].w);
            const uint32_t nb = group_reduce<OpMaxU>(T::absmax_finish(mm.absacc), ga.gv);
            const uint32_t umx = group_reduce<OpMaxF>(as_u(mm.mx), ga.gv), umn = group_reduce<OpMinF>(as_u(mm.mn), ga.gv);
            if (i == 0) {
                lane_nb = nb, lane_mx = umx, lane_mn = umn;
            } else {
                lane_nb = OpMaxU::f(lane_nb, nb), lane_mx = OpMaxF::f(lane_mx, umx), lane_mn = OpMinF::f(lane_mn, umn);
            }
            float mx = as_f(umx), mn = as_f(umn);
            if (absbits_is_nan(nb)) mx = mn = as_f(0x7FC00000u);  // torch.max/min propagate NaN
            ar[i] = asym_row<DT>(mx, mn, a.asym);
        }
        if (want_bounds) {
            block_reduce3<OpMaxU, OpMaxF, OpMinF, NW>(lane_nb, lane_mx, lane_mn, red);
            ub = as_f(lane_mx), lb = as_f(lane_mn);
            if (absbits_is_nan(lane_nb)) ub = lb = as_f(0x7FC00000u);
            if (t == 0) store_bounds(a.bounds, row, ub, lb);
        }
    }

    // Elementwise pass.  Rows that can actually be clipped also emit the STE bit mask for the backward (full-row layout).
    const bool want_mask = a.mask && !cannot_clip(ub, lb, a.lo, a.hi);  // wave-uniform
    const bool sym_clip = a.lo == -a.hi;
    const uint32_t clipk = (ub != ub) ? 0u : a.clipk;  // a row with a NaN compares as floats (NaN passes the gradient)
    uint8_t* mrow = (uint8_t*)(a.mask + row * a.mask_row_words);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int v = t + i * TPR;
        const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
        float f[EPV];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            float fd[T::EPD];
            T::unpack(w[d], fd);
#pragma unroll
            for (int k = 0; k < T::EPD; ++k) f[d * T::EPD + k] = fd[k];
        }
        if (want_mask) ste_mask_record<DT>(mrow, v, v < nvec, r[i], f, a.lo, a.hi, sym_clip, clipk);
        uint32_t o[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            float fd[T::EPD];
#pragma unroll
            for (int k = 0; k < T::EPD; ++k) fd[k] = f[d * T::EPD + k];
            if constexpr (AC != 0) {  // fp32 arithmetic behind the reciprocal, rounded once to the tensor dtype
#pragma unroll
                for (int k = 0; k < T::EPD; ++k) fd[k] = sym_elem_autocast(fd[k], sr[i]);
                o[d] = T::pack(fd);
            } else if constexpr (!ASYM) {
                o[d] = sym_chain<DT, FAST>(fd, sr[i], nullptr);
            } else {
                o[d] = asym_chain<DT, AFAST>(fd, ar[i], a.asym, nullptr);   // (fp16: no per-row LDS table -- it does not fit a group)
            }
        }
        if (v < nvec) st16<true>(&yr[v], make_uint4(o[0], o[1], o[2], o[3]));
    }
}

// launch shapes: by_group_shape (fq_shapes.h), a ladder of its own because every rung must hold whole groups
template <int DT, bool ASYM, bool FAST, int AC>
static void launch_group_shape(const RowArgs& a, int64_t nvec, GroupArgs ga, hipStream_t st) {
    by_group_shape(nvec, [&](auto tpr, auto vpt) {
        constexpr int TPR = decltype(tpr)::value, VPT = decltype(vpt)::value;
        launch_rows<TPR>(group_reg_kernel<DT, TPR, VPT, ASYM, FAST, AC>, a.rows, st, a, ga);
    });
}

// a: x / y / rows / cols / sym / asym constants and (training mode) bounds + mask, validated by fq_group_fwd; gv: vectors per group
template <int DT> int launch_group(bool asym, bool fast, int autocast, RowArgs a, int gv, hipStream_t st) {
    using T = Ty<DT>;
    constexpr int EPV = 16 / T::ESIZE;
    const int64_t nvec = a.cols / EPV;
    GroupArgs ga{gv, a.rows * a.cols * T::ESIZE >= NT_LOAD_MIN_BYTES ? 1 : 0};
    begin_launches();
    if constexpr (T::ESIZE == 2) {
        if (autocast) {
            launch_group_shape<DT, false, false, 1>(a, nvec, ga, st);
            return launch_result();
        }
    }
    if constexpr (DT == BF16) {   // reciprocal multiplies instead of IEEE divides: the row-wise argument holds per scale value
        if (fast) {
            if (asym) launch_group_shape<DT, true, true, 0>(a, nvec, ga, st);
            else launch_group_shape<DT, false, true, 0>(a, nvec, ga, st);
            return launch_result();
        }
        if (!asym) return fail(FQ_ERR_ARG, "internal: bf16 Sym always takes the reciprocal form");
    }
    if (asym) launch_group_shape<DT, true, false, 0>(a, nvec, ga, st);
    else if constexpr (DT != BF16) launch_group_shape<DT, false, false, 0>(a, nvec, ga, st);
    return launch_result();
}

#define FQ_INSTANTIATE_GROUP(DT) template int launch_group<DT>(bool, bool, int, RowArgs, int, hipStream_t);

}  // namespace fq
