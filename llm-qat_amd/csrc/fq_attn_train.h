// fq_attn_train.h -- the backward of the fused training attention: the kernels behind
// include/llmqat_fakequant_attn_train.h.  The forward is fq_attn_prefill.h's pre_kernel with its STATS output.
//
//   out = softmax(max(rb(rb(q k^T) inv) + mask, finfo.min), -1) v        ->  dq, dk, dv from dout, with no [B, H, T, S] tensor
//
// Arithmetic.  Everything in front of the softmax is recomputed by the forward's device functions: x = rb(q k^T), a = attn_a(x, mask,
// inv), z = attn_z(a), p = attn_p(z, loss_ref(m), 1 / l) from the saved (m, l).  Then, all in fp32 and unrounded: g = dout . v,
// delta = sum_s p g (NOT sum_d dout out: the rounding of `out` leaves an error of u sum_d |dout out| in that form, which a v with a common
// sign makes many times u sum_s p |g|, the error the composed path has; measured), d = (g - delta) p, times
// torch.max's gradient under a mask (1 where a > MIN_P, 1/2 where a == MIN_P, 0 below, a NaN a passes), times inv.  TWO roundings to the dtype stand in the backward, both in front of a matrix instruction that needs a
// 16-bit operand: rb(p) for dv = sum_t rb(p) dout, and ds = rb(d inv) for dq = sum_s ds k and dk = sum_t ds q.  The sums are fp32 and
// each output is rounded once.  Keys that a row does not see (past S, past the causal diagonal) have p = 0 and ds = 0 exactly.
//
// Work split: two launches, no atomics, every output written once.
//   trn_dq_kernel   grid (query tiles, B * H), the forward's split.  A workgroup of TRN_WAVES waves owns TRN_DQ_QT query rows and walks
//                   the keys in tiles of TRN_DQ_KT through two LDS buffers (K and V, as the forward).  A wave holds q and dout of its
//                   RB 16-row blocks in registers as B operands.  It walks the keys TWICE: the first walk adds up delta of its rows (the
//                   lane's share over its keys, then the four lane groups) and writes it to the workspace for the second launch; the
//                   second walk makes ds and dq.  `out` is not read.
//                   Per tile: S^T = K q^T and dP^T = V dout^T (A from LDS with 16-byte reads: lane (j, g) holds keys 4 g + r of query
//                   j), ds per element with the lane's own (m, l, delta), dQ^T += K^T ds^T (A = K^T by the transposing LDS read the
//                   forward uses for V^T, two 16-key tiles as the B operand under the forward's k order).
//   trn_dkv_kernel  behind it on the same stream, its mirror: grid (key tiles, B * H).  A wave holds K and V of its KB 16-key blocks in
//                   registers as B operands; the workgroup walks the query rows in tiles of TRN_DKV_QT, staging q, dout and the rows'
//                   (loss_ref(m), 1 / l, delta) through two LDS buffers.  S = q K^T and dP = dout V^T: lane (j, g) holds queries
//                   4 g + r of key j.  dV^T += dout^T rb(p) and dK^T += q^T ds, A = dout^T and q^T by the transposing read; p and ds
//                   never leave registers.  The mask is read with element loads here: a lane's eight elements lie in eight rows.
//
// Causal mode: the dq kernel visits no key tile past its workgroup's last row (a wave none past its own); the dk/dv kernel starts its
// walk at the first query tile that sees the workgroup's first key (a wave skips tiles in front of its own first key), and key tile 0,
// the longest, is block 0.
//
// Guards, as the forward's.  Rows >= T and keys >= S clamp their addresses, have zero q / dout / k / v fragments and p = 0 behind the
// clamp, so they add exactly 0, and they store nothing.  64-bit indices.
#pragma once
#include "fq_attn_prefill.h"

namespace fq {

struct TrnArgs {
    const void* q;       // [B, H, T, D] by strides (batch, head, token; last stride 1)
    const void* k;       // [B, H, S, D] likewise
    const void* v;
    const void* mask;    // [B, 1, T, S] by (batch, row) stride, or nullptr
    const void* out;     // [B, H, T, D] by strides: the forward's result
    const void* dout;    // [B, H, T, D] by strides: its gradient
    const float* stats;  // [B, H, T, 2]: the forward's (m, l)
    float* delta;        // [B, H, T]: written by the dq kernel, read by the dk/dv kernel
    void* dq;            // [B, T, H, D] contiguous
    void* dk;            // [B, S, H, D] contiguous
    void* dv;
    int64_t qs[3], ks[3], vs[3], os[3], gs[3];
    int64_t mbs, mrs;
    int64_t H, T, S;
    float inv;
};

// p of one (query, key), and a, the chain's value in front of the clamp: acc is the first product's fp32 sum, mk the mask's element;
// seen: the row sees the key
template <int DT, int MDT> __device__ __forceinline__ float trn_p(float acc, float mk, float ref, float rinv, float inv, bool seen, float& a) {
    const float x = Ty<DT>::rb(acc);                        // the first product's own rounding
    a = attn_a<DT, MDT>(x, mk, inv);
    return seen ? attn_p(attn_z<DT, MDT>(a), ref, rinv) : 0.0f;
}
// p and ds of one (query, key); g = dout . v
template <int DT, int MDT>
__device__ __forceinline__ void trn_elem(float acc, float mk, float g, float ref, float rinv, float delta, float inv, bool seen, float& p, float& ds) {
    float a;
    p = trn_p<DT, MDT>(acc, mk, ref, rinv, inv, seen, a);
    float d = (g - delta) * p;
    if constexpr (MDT != ATTN_NOMASK) {
        const float mn = attn_min<attn_sum_dtype<DT, MDT>()>();
        d = a == mn ? d * 0.5f : (a < mn ? 0.0f : d);       // a NaN a compares false twice: d passes
    }
    ds = seen ? d * inv : 0.0f;
}

// eight values of a lane as the B operand of a 16x16x32 instruction under the k order of fq_attn_prefill.h, rounded to the dtype
template <int DT> __device__ __forceinline__ u32x4_t trn_pack8(const float (&f)[8]) {
    u32x4_t r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float e[2] = {f[2 * i], f[2 * i + 1]};
        r[i] = Ty<DT>::pack(e);
    }
    return r;
}

// A = X^T for 16 columns of d from a staged [32, D] tile: lane (j, g) receives X[row(g, c), 16 db + j], c = 0 .. 7 (fq_attn_prefill.h, V)
__device__ __forceinline__ u32x4_t trn_read_tr(const char* tile, int rs, int db, int j, int g) {
    typedef __attribute__((address_space(3))) i16x4_t* lds_i16x4_ptr;
    const char* p0 = tile + (4 * g + (j >> 2)) * rs + 2 * (16 * db + 4 * (j & 3));
    const i16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(uintptr_t)p0);
    const i16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(uintptr_t)(p0 + 16 * rs));
    return __builtin_bit_cast(u32x4_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int DT, int MDT, bool CAUSAL, int D, int RB, bool VEC, bool MVEC>
__global__ __launch_bounds__(TRN_WAVES * 64, 2) void trn_dq_kernel(TrnArgs a) {
    static_assert(D == 64 || D == 128, "head sizes served");
    static_assert(!CAUSAL || MDT == ATTN_NOMASK, "the causal mode reads no mask");
    static_assert(TRN_DQ_KT == 32, "a key tile is two 16-key score tiles: the k of one matrix instruction");
    constexpr int KT = TRN_DQ_KT;
    constexpr int KS = D / 32;
    constexpr int DB = D / 16;
    constexpr int RS = pre_row_bytes<D>();
    constexpr int TILE = KT * RS;
    constexpr int LPR = D / 8;
    constexpr int RPP = TRN_WAVES * 64 / LPR;
    constexpr int NLI = KT / RPP;
    constexpr int QT = TRN_WAVES * 16 * RB;
    static_assert(NLI >= 1 && NLI * RPP == KT, "the workgroup's passes cover a tile exactly");
    __shared__ __attribute__((aligned(16))) char smem[2][2][TILE];      // [buffer][K, V]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int64_t qt = (int64_t)gridDim.x - 1 - blockIdx.x;             // the last query tile (in causal mode the longest) first
    const int64_t bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    const int64_t T = a.T, S = a.S, last = S - 1;
    const int64_t q0 = qt * QT, w0 = q0 + wave * (16 * RB);

    int64_t nt = (S + KT - 1) / KT;
    int64_t wnt = w0 < T ? nt : 0;
    if constexpr (CAUSAL) {
        const int64_t tl = (q0 + QT < T ? q0 + QT : T) - 1, wl = (w0 + 16 * RB < T ? w0 + 16 * RB : T) - 1;
        nt = (S - T + tl) / KT + 1;
        wnt = w0 < T ? (S - T + wl) / KT + 1 : 0;
    }

    const uint16_t* kp = (const uint16_t*)a.k + b * a.ks[0] + h * a.ks[1] + 8 * (tid % LPR);
    const uint16_t* vp = (const uint16_t*)a.v + b * a.vs[0] + h * a.vs[1] + 8 * (tid % LPR);
    const int lrow = tid / LPR, lcol = 16 * (tid % LPR);

    u32x4_t qf[RB][KS], gf[RB][KS];
    int64_t mb[RB], lim[RB], trow[RB];
    float ref[RB], rinv[RB], dl[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int64_t t = w0 + 16 * rb + j, tq = t < T ? t : T - 1;
        trow[rb] = t;
        mb[rb] = MDT == ATTN_NOMASK ? 0 : b * a.mbs + tq * a.mrs;
        lim[rb] = CAUSAL && S - T + t < last ? S - T + t : last;
        const uint16_t* qp = (const uint16_t*)a.q + b * a.qs[0] + h * a.qs[1] + tq * a.qs[2] + 8 * g;
        const uint16_t* gp = (const uint16_t*)a.dout + b * a.gs[0] + h * a.gs[1] + tq * a.gs[2] + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const u32x4_t x = dec_ld16<VEC>(qp + 32 * ks), y = dec_ld16<VEC>(gp + 32 * ks);
            qf[rb][ks] = t < T ? x : (u32x4_t){0u, 0u, 0u, 0u};
            gf[rb][ks] = t < T ? y : (u32x4_t){0u, 0u, 0u, 0u};
        }
        const int64_t row = (b * a.H + h) * T + tq;
        ref[rb] = loss_ref(a.stats[2 * row]);
        rinv[rb] = 1.0f / a.stats[2 * row + 1];
        dl[rb] = 0.0f;
    }

    auto load_tile = [&](int64_t tile, u32x4_t(&kr)[NLI], u32x4_t(&vr)[NLI]) {
#pragma unroll
        for (int it = 0; it < NLI; ++it) {
            int64_t key = tile * KT + it * RPP + lrow;
            key = key < last ? key : last;
            kr[it] = dec_ld16<VEC>(kp + key * a.ks[2]);
            vr[it] = dec_ld16<VEC>(vp + key * a.vs[2]);
        }
    };
    auto store_tile = [&](int buf, const u32x4_t(&kr)[NLI], const u32x4_t(&vr)[NLI]) {
#pragma unroll
        for (int it = 0; it < NLI; ++it) {
            *(u32x4_t*)(smem[buf][0] + (it * RPP + lrow) * RS + lcol) = kr[it];
            *(u32x4_t*)(smem[buf][1] + (it * RPP + lrow) * RS + lcol) = vr[it];
        }
    };

    f32x4_t acc[RB][DB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
#pragma unroll
        for (int i = 0; i < DB; ++i) acc[rb][i] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
    }

    // one walk over the key tiles.  The first adds up the lane's share of delta = sum_s p g; the second, with delta known, makes ds and dq
    auto walk = [&](auto second) {
    constexpr bool SECOND = decltype(second)::value != 0;
    u32x4_t kr[NLI], vr[NLI];
    load_tile(0, kr, vr);
    store_tile(0, kr, vr);
    __syncthreads();
    for (int64_t tile = 0; tile < nt; ++tile) {
        const int buf = (int)(tile & 1);
        const bool more = tile + 1 < nt;
        if (more) load_tile(tile + 1, kr, vr);
        if (tile < wnt) {
            const char* kt = smem[buf][0];
            const char* vt = smem[buf][1];
            const int64_t k0 = tile * KT + 4 * g;                        // the lane's keys: k0 + 16 (c >> 2) + (c & 3)
            float mk[RB][8];
            if constexpr (MDT != ATTN_NOMASK) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    pre_mask4<MDT, MVEC>(a.mask, mb[rb], k0, last, &mk[rb][0]);
                    pre_mask4<MDT, MVEC>(a.mask, mb[rb], k0 + 16, last, &mk[rb][4]);
                }
            }
            f32x4_t sc[RB][2], dp[RB][2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) sc[rb][hf] = dp[rb][hf] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4_t kf = *(const u32x4_t*)(kt + (16 * hf + j) * RS + 2 * (32 * ks + 8 * g));
                    const u32x4_t vf = *(const u32x4_t*)(vt + (16 * hf + j) * RS + 2 * (32 * ks + 8 * g));
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) {
                        sc[rb][hf] = dec_mfma<DT>(kf, qf[rb][ks], sc[rb][hf]);
                        dp[rb][hf] = dec_mfma<DT>(vf, gf[rb][ks], dp[rb][hf]);
                    }
                }
            }
            u32x4_t sf[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                float ds[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int64_t key = k0 + 16 * (c >> 2) + (c & 3);
                    const float mc = MDT == ATTN_NOMASK ? 0.0f : mk[rb][c], gc = dp[rb][c >> 2][c & 3];
                    float p, av;
                    if constexpr (SECOND) {
                        trn_elem<DT, MDT>(sc[rb][c >> 2][c & 3], mc, gc, ref[rb], rinv[rb], dl[rb], a.inv, key <= lim[rb], p, ds[c]);
                    } else {
                        p = trn_p<DT, MDT>(sc[rb][c >> 2][c & 3], mc, ref[rb], rinv[rb], a.inv, key <= lim[rb], av);
                        dl[rb] += key <= lim[rb] ? p * gc : 0.0f;
                    }
                }
                if constexpr (SECOND) sf[rb] = trn_pack8<DT>(ds);
            }
            if constexpr (SECOND) {
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const u32x4_t ktf = trn_read_tr(kt, RS, db, j, g);
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) acc[rb][db] = dec_mfma<DT>(ktf, sf[rb], acc[rb][db]);
                }
            }
        }
        if (more) store_tile(buf ^ 1, kr, vr);
        __syncthreads();
    }
    };
    walk(Const<0>{});
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        dl[rb] = dec_sum_groups(dl[rb]);
        if (trow[rb] < T && g == 0) a.delta[(b * a.H + h) * T + trow[rb]] = dl[rb];
    }
    walk(Const<1>{});

#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        if (trow[rb] < T) {
            const int64_t o = ((b * T + trow[rb]) * a.H + h) * D + 4 * g;
#pragma unroll
            for (int db = 0; db < DB; ++db) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Ty<DT>::store1(a.dq, o + 16 * db + r, acc[rb][db][r]);
            }
        }
    }
}

template <int DT, int MDT, bool CAUSAL, int D, int KB, bool VEC>
__global__ __launch_bounds__(TRN_WAVES * 64, 2) void trn_dkv_kernel(TrnArgs a) {
    static_assert(D == 64 || D == 128, "head sizes served");
    static_assert(!CAUSAL || MDT == ATTN_NOMASK, "the causal mode reads no mask");
    static_assert(TRN_DKV_QT == 32, "a query tile is two 16-row score tiles: the k of one matrix instruction");
    constexpr int QT = TRN_DKV_QT;
    constexpr int KS = D / 32;
    constexpr int DB = D / 16;
    constexpr int RS = pre_row_bytes<D>();
    constexpr int TILE = QT * RS;
    constexpr int LPR = D / 8;
    constexpr int RPP = TRN_WAVES * 64 / LPR;
    constexpr int NLI = QT / RPP;
    constexpr int KT = TRN_WAVES * 16 * KB;
    static_assert(NLI >= 1 && NLI * RPP == QT, "the workgroup's passes cover a tile exactly");
    __shared__ __attribute__((aligned(16))) char smem[2][2][TILE];      // [buffer][q, dout]
    __shared__ __attribute__((aligned(16))) float srow[2][3][QT];       // [buffer][loss_ref(m), 1 / l, delta]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int64_t kt = blockIdx.x;                                      // key tile 0 (in causal mode the longest) first
    const int64_t bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    const int64_t T = a.T, S = a.S, last = S - 1;
    const int64_t k0 = kt * KT, w0 = k0 + wave * (16 * KB);
    const int64_t past = S - T;                                         // causal: row t sees the keys s <= past + t

    const int64_t nt = (T + QT - 1) / QT;
    int64_t t0 = 0, wq = 0;                                             // the first tile of the walk; the first row the wave's keys are seen by
    if constexpr (CAUSAL) {
        t0 = (k0 > past ? k0 - past : 0) / QT;
        wq = w0 > past ? w0 - past : 0;
    }

    const uint16_t* qp = (const uint16_t*)a.q + b * a.qs[0] + h * a.qs[1] + 8 * (tid % LPR);
    const uint16_t* gp = (const uint16_t*)a.dout + b * a.gs[0] + h * a.gs[1] + 8 * (tid % LPR);
    const int lrow = tid / LPR, lcol = 16 * (tid % LPR);
    const int64_t srow0 = (b * a.H + h) * T;

    u32x4_t kf[KB][KS], vf[KB][KS];
    int64_t key[KB], kc[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        key[kb] = w0 + 16 * kb + j;
        kc[kb] = key[kb] < last ? key[kb] : last;
        const uint16_t* kp = (const uint16_t*)a.k + b * a.ks[0] + h * a.ks[1] + kc[kb] * a.ks[2] + 8 * g;
        const uint16_t* vp = (const uint16_t*)a.v + b * a.vs[0] + h * a.vs[1] + kc[kb] * a.vs[2] + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const u32x4_t x = dec_ld16<VEC>(kp + 32 * ks), y = dec_ld16<VEC>(vp + 32 * ks);
            kf[kb][ks] = key[kb] < S ? x : (u32x4_t){0u, 0u, 0u, 0u};
            vf[kb][ks] = key[kb] < S ? y : (u32x4_t){0u, 0u, 0u, 0u};
        }
    }

    auto load_tile = [&](int64_t tile, u32x4_t(&qr)[NLI], u32x4_t(&gr)[NLI], float(&sr)[3]) {
#pragma unroll
        for (int it = 0; it < NLI; ++it) {
            const int64_t t = tile * QT + it * RPP + lrow, tq = t < T ? t : T - 1;
            const u32x4_t x = dec_ld16<VEC>(qp + tq * a.qs[2]), y = dec_ld16<VEC>(gp + tq * a.gs[2]);
            qr[it] = t < T ? x : (u32x4_t){0u, 0u, 0u, 0u};
            gr[it] = t < T ? y : (u32x4_t){0u, 0u, 0u, 0u};
        }
        if (tid < QT) {
            const int64_t t = tile * QT + tid, tq = t < T ? t : T - 1;
            const float m = a.stats[2 * (srow0 + tq)], l = a.stats[2 * (srow0 + tq) + 1], d = a.delta[srow0 + tq];
            sr[0] = loss_ref(m), sr[1] = 1.0f / l, sr[2] = t < T ? d : 0.0f;
        }
    };
    auto store_tile = [&](int buf, const u32x4_t(&qr)[NLI], const u32x4_t(&gr)[NLI], const float(&sr)[3]) {
#pragma unroll
        for (int it = 0; it < NLI; ++it) {
            *(u32x4_t*)(smem[buf][0] + (it * RPP + lrow) * RS + lcol) = qr[it];
            *(u32x4_t*)(smem[buf][1] + (it * RPP + lrow) * RS + lcol) = gr[it];
        }
        if (tid < QT) {
#pragma unroll
            for (int i = 0; i < 3; ++i) srow[buf][i][tid] = sr[i];
        }
    };

    f32x4_t dk[KB][DB], dv[KB][DB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int i = 0; i < DB; ++i) dk[kb][i] = dv[kb][i] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
    }

    u32x4_t qr[NLI], gr[NLI];
    float sr[3] = {0.0f, 0.0f, 0.0f};
    load_tile(t0, qr, gr, sr);
    store_tile((int)(t0 & 1), qr, gr, sr);
    __syncthreads();
    for (int64_t tile = t0; tile < nt; ++tile) {
        const int buf = (int)(tile & 1);
        const bool more = tile + 1 < nt;
        if (more) load_tile(tile + 1, qr, gr, sr);
        const int64_t q0 = tile * QT;
        if (w0 < S && q0 + QT > wq) {
            const char* qtile = smem[buf][0];
            const char* gtile = smem[buf][1];
            f32x4_t sc[KB][2], dp[KB][2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) sc[kb][hf] = dp[kb][hf] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4_t qa = *(const u32x4_t*)(qtile + (16 * hf + j) * RS + 2 * (32 * ks + 8 * g));
                    const u32x4_t ga = *(const u32x4_t*)(gtile + (16 * hf + j) * RS + 2 * (32 * ks + 8 * g));
#pragma unroll
                    for (int kb = 0; kb < KB; ++kb) {
                        sc[kb][hf] = dec_mfma<DT>(qa, kf[kb][ks], sc[kb][hf]);
                        dp[kb][hf] = dec_mfma<DT>(ga, vf[kb][ks], dp[kb][hf]);
                    }
                }
            }
            // the lane's rows: q0 + 16 (c >> 2) + 4 g + (c & 3)
            f32x4_t rr[2], ri[2], rd[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                rr[hf] = *(const f32x4_t*)&srow[buf][0][16 * hf + 4 * g];
                ri[hf] = *(const f32x4_t*)&srow[buf][1][16 * hf + 4 * g];
                rd[hf] = *(const f32x4_t*)&srow[buf][2][16 * hf + 4 * g];
            }
            u32x4_t pf[KB], sf[KB];
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                float p[8], ds[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int64_t t = q0 + 16 * (c >> 2) + 4 * g + (c & 3), tq = t < T ? t : T - 1;
                    float mk = 0.0f;
                    if constexpr (MDT != ATTN_NOMASK) mk = Ty<MDT>::load1(a.mask, b * a.mbs + tq * a.mrs + kc[kb]);
                    const bool seen = t < T && key[kb] < S && (!CAUSAL || key[kb] <= past + t);
                    trn_elem<DT, MDT>(sc[kb][c >> 2][c & 3], mk, dp[kb][c >> 2][c & 3], rr[c >> 2][c & 3], ri[c >> 2][c & 3], rd[c >> 2][c & 3],
                                      a.inv, seen, p[c], ds[c]);
                }
                pf[kb] = trn_pack8<DT>(p);
                sf[kb] = trn_pack8<DT>(ds);
            }
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                const u32x4_t gtf = trn_read_tr(gtile, RS, db, j, g);
                const u32x4_t qtf = trn_read_tr(qtile, RS, db, j, g);
#pragma unroll
                for (int kb = 0; kb < KB; ++kb) {
                    dv[kb][db] = dec_mfma<DT>(gtf, pf[kb], dv[kb][db]);
                    dk[kb][db] = dec_mfma<DT>(qtf, sf[kb], dk[kb][db]);
                }
            }
        }
        if (more) store_tile(buf ^ 1, qr, gr, sr);
        __syncthreads();
    }

#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
        if (key[kb] < S) {
            const int64_t o = ((b * S + key[kb]) * a.H + h) * D + 4 * g;
#pragma unroll
            for (int db = 0; db < DB; ++db) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    Ty<DT>::store1(a.dk, o + 16 * db + r, dk[kb][db][r]);
                    Ty<DT>::store1(a.dv, o + 16 * db + r, dv[kb][db][r]);
                }
            }
        }
    }
}

}  // namespace fq
