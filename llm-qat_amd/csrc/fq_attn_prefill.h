// fq_attn_prefill.h -- the fused prefill attention: the kernel behind include/llmqat_fakequant_attn_prefill.h.
//
//   out[b, t, h, :] = softmax(max(rb(rb(q k^T) inv) + mask, finfo.min), -1) v        for any T >= 1 query rows against S keys
//
// in ONE kernel: no [B, H, T, S] tensor exists in any precision.  The arithmetic is the decode kernel's (fq_attn_decode.h): section 29's
// chain with the two products around it, the per-element roundings by that section's device functions (attn_a, attn_z, attn_exp), an
// online fp32 softmax per query row, the unnormalised exponentials rounded to the dtype as the second product's operand, one fp32
// division in front of the one output rounding.
//
// Work split.  Grid (query tiles, B * H), the longest query tiles first.  A workgroup of PRE_WAVES waves owns PRE_QT query rows and
// walks ALL keys in tiles of PRE_KT: no split along S, no workspace, no merge.  Wave w owns rows [16 RB w, 16 RB (w + 1)) of the tile
// as RB blocks of 16 rows (RB = PRE_RPW / 16), each with (m, l) and an fp32 [16, D] accumulator in registers.
//
// Data movement (v_mfma_f32_16x16x32_{bf16,f16}; lane = 16 g + j).
//   K, V     the workgroup loads each PRE_KT x D tile of K and of V ONCE into LDS (16-byte global loads, rows padded by 16 bytes) and
//            its four waves share it.  Two LDS buffers: the next tile's global loads are issued in front of this tile's matrix work and
//            stored behind it, one barrier per tile.
//   scores   S^T = K q^T.  A = 16 keys of K from LDS: lane (j, g) reads the 16 bytes of key row j at d = 32 ks + 8 g; every A fragment
//            feeds the RB q blocks of the wave.  B = q, held in registers for the whole walk, rows >= T zero.  The result registers
//            hold keys 4 g + r of query row j.
//   P        two 16-key score tiles are a B operand of the PV instruction under the k order  k = 8 g + c  <->  key (c < 4 ? 4 g + c :
//            16 + 4 g + c - 4), as in the decode kernel.  P never leaves registers; the softmax factors of a row are the lane's own.
//   V        A = V^T, 16 columns of d per instruction: lane (j, g) needs V[key(g, c), 16 db + j], c = 0 .. 7.  PRE_V_TR = 1: two
//            transposing reads (ds_read_b64_tr_b16): in each group of 16 lanes, lane i addresses the 8 bytes at d = 16 db + 4 (i % 4)
//            of key row 4 g + i / 4 (and 16 rows further for the second), and receives the four keys of column 16 db + i.
//            PRE_V_TR = 0: the decode kernel's eight 2-byte reads into the same registers.  Every V fragment feeds the RB blocks.
//   mask     straight from global memory: a lane's four consecutive keys as one 16-byte (fp32) or 8-byte (16-bit) load where the base
//            and the strides allow and the four keys exist, element loads otherwise.
//
// Causal mode (CAUSAL, no mask pointer, T <= S): query row t sees keys s <= S - T + t, the others have weight exactly 0 (-inf in front
// of the exponential, no clamp: the no-mask chain).  Key tiles past the workgroup's last row are not visited, and a wave does no matrix
// work on tiles past its own last row.
//
// Guards.  Query rows >= T use row T - 1's addresses, have zero q and store nothing.  A key past S clamps its row index on every load
// and is -inf behind the clamp.  The reference point of a maximum of -inf is 0 (loss_ref) and the old maximum enters exp() raw.  A NaN
// or +inf score makes its row's sum NaN and nothing else: query rows are columns of both matrix instructions.  64-bit indices.
#pragma once
#include "fq_attn_decode.h"

#ifndef PRE_V_TR
#define PRE_V_TR 1         // the transposing LDS read for V^T; 0: 2-byte reads (DESIGN.md section 31 has both forms' times)
#endif

namespace fq {

typedef short i16x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

struct PreArgs {
    const void* q;       // [B, H, T, D] by strides (batch, head, token; last stride 1)
    const void* k;       // [B, H, S, D] likewise
    const void* v;
    const void* mask;    // [B, 1, T, S] by (batch, row) stride, or nullptr
    void* out;           // [B, T, H, D] contiguous
    int64_t qs[3], ks[3], vs[3];
    int64_t mbs, mrs;
    int64_t H, T, S;
    float inv;
    int64_t G;           // query heads of a K/V head, read by the GQA instantiations alone (fq_attn_gqa.hip): k, v are [B, H / G, S, D]
    float* stats;        // [B, H, T, 2]: (m, l) of each real row; read by the STATS instantiations alone (fq_attn_train.hip), nullptr: not written
};

// the mask of four consecutive keys from key0 (a multiple of 4) of the row at element `base`; keys past `last` repeat the last one's
template <int MDT, bool MVEC> __device__ __forceinline__ void pre_mask4(const void* p, int64_t base, int64_t key0, int64_t last, float* m) {
    if (MVEC && key0 + 3 <= last) {
        if constexpr (MDT == F32) {
            const f32x4_t x = *(const f32x4_t*)((const float*)p + base + key0);
#pragma unroll
            for (int i = 0; i < 4; ++i) m[i] = x[i];
        } else {
            const u32x2_t x = *(const u32x2_t*)((const uint16_t*)p + base + key0);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float e[2];
                Ty<MDT>::unpack(x[i], e);
                m[2 * i] = e[0], m[2 * i + 1] = e[1];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t key = key0 + i < last ? key0 + i : last;
            m[i] = Ty<MDT>::load1(p, base + key);
        }
    }
}

template <int D> constexpr int pre_row_bytes() { return 2 * D + 16; }

// MDT: the mask's dtype or ATTN_NOMASK; CAUSAL only beside ATTN_NOMASK.  RB: 16-row blocks of a wave.  VEC / MVEC: 16-byte loads of
// q, k, v / vector loads of the mask.  STATS: the row's maximum and the group-reduced sum go to a.stats behind the walk (the training forward)
// GQA: K and V come from head h / a.G; nothing else moves
template <int DT, int MDT, bool CAUSAL, int D, int RB, bool VEC, bool MVEC, bool STATS = false, bool GQA = false>
__global__ __launch_bounds__(PRE_WAVES * 64, 2) void pre_kernel(PreArgs a) {
    static_assert(D == 64 || D == 128, "head sizes served");
    static_assert(!CAUSAL || MDT == ATTN_NOMASK, "the causal mode reads no mask");
    static_assert(PRE_KT == 32, "a key tile is two 16-key score tiles: the k of one PV instruction");
    constexpr int KS = D / 32;                          // k-steps of a score tile
    constexpr int DB = D / 16;                          // 16-column blocks of the output
    constexpr int RS = pre_row_bytes<D>();
    constexpr int TILE = PRE_KT * RS;                   // bytes of one staged tile
    constexpr int LPR = D / 8;                          // threads of a row (16 bytes each)
    constexpr int RPP = PRE_WAVES * 64 / LPR;           // rows of one pass of the workgroup
    constexpr int NLI = PRE_KT / RPP;                   // passes (load instructions of a thread) per tile and tensor
    constexpr int QT = PRE_WAVES * 16 * RB;
    static_assert(NLI >= 1 && NLI * RPP == PRE_KT, "the workgroup's passes cover a tile exactly");
    __shared__ __attribute__((aligned(16))) char smem[2][2][TILE];      // [buffer][K, V]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int64_t qt = (int64_t)gridDim.x - 1 - blockIdx.x;             // the last query tile (under a causal mask the longest) first
    const int64_t bh = blockIdx.y, b = bh / a.H, h = bh % a.H;
    const int64_t T = a.T, S = a.S, last = S - 1;
    const int64_t q0 = qt * QT, w0 = q0 + wave * (16 * RB);

    int64_t nt = (S + PRE_KT - 1) / PRE_KT;             // tiles the workgroup walks
    int64_t wnt = w0 < T ? nt : 0;                      // tiles the wave has matrix work on
    if constexpr (CAUSAL) {
        const int64_t tl = (q0 + QT < T ? q0 + QT : T) - 1, wl = (w0 + 16 * RB < T ? w0 + 16 * RB : T) - 1;
        nt = (S - T + tl) / PRE_KT + 1;
        wnt = w0 < T ? (S - T + wl) / PRE_KT + 1 : 0;
    }

    const int64_t kvh = GQA ? h / a.G : h;
    const uint16_t* kp = (const uint16_t*)a.k + b * a.ks[0] + kvh * a.ks[1] + 8 * (tid % LPR);
    const uint16_t* vp = (const uint16_t*)a.v + b * a.vs[0] + kvh * a.vs[1] + 8 * (tid % LPR);
    const int lrow = tid / LPR, lcol = 16 * (tid % LPR);

    u32x4_t qf[RB][KS];
    int64_t mb[RB], lim[RB], trow[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int64_t t = w0 + 16 * rb + j, tq = t < T ? t : T - 1;
        trow[rb] = t;
        mb[rb] = MDT == ATTN_NOMASK ? 0 : b * a.mbs + tq * a.mrs;
        lim[rb] = CAUSAL && S - T + t < last ? S - T + t : last;        // the last key the row sees
        const uint16_t* qp = (const uint16_t*)a.q + b * a.qs[0] + h * a.qs[1] + tq * a.qs[2] + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const u32x4_t x = dec_ld16<VEC>(qp + 32 * ks);
            qf[rb][ks] = t < T ? x : (u32x4_t){0u, 0u, 0u, 0u};
        }
    }

    auto load_tile = [&](int64_t tile, u32x4_t(&kr)[NLI], u32x4_t(&vr)[NLI]) {
#pragma unroll
        for (int it = 0; it < NLI; ++it) {
            int64_t key = tile * PRE_KT + it * RPP + lrow;
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

    float m[RB], l[RB];
    f32x4_t acc[RB][DB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        m[rb] = LOSS_NEG_INF, l[rb] = 0.0f;
#pragma unroll
        for (int i = 0; i < DB; ++i) acc[rb][i] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
    }

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
            const int64_t k0 = tile * PRE_KT + 4 * g;                    // the lane's keys: k0 + 16 (c >> 2) + (c & 3)
            float mk[RB][8];
            if constexpr (MDT != ATTN_NOMASK) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    pre_mask4<MDT, MVEC>(a.mask, mb[rb], k0, last, &mk[rb][0]);
                    pre_mask4<MDT, MVEC>(a.mask, mb[rb], k0 + 16, last, &mk[rb][4]);
                }
            }
            f32x4_t sc[RB][2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) sc[rb][hf] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const u32x4_t kf = *(const u32x4_t*)(kt + (16 * hf + j) * RS + 2 * (32 * ks + 8 * g));
#pragma unroll
                    for (int rb = 0; rb < RB; ++rb) sc[rb][hf] = dec_mfma<DT>(kf, qf[rb][ks], sc[rb][hf]);
                }
            }
            u32x4_t pf[RB];
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                float z[8];
                float tmax = LOSS_NEG_INF;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int64_t key = k0 + 16 * (c >> 2) + (c & 3);
                    const float x = Ty<DT>::rb(sc[rb][c >> 2][c & 3]);      // the first product's own rounding
                    const float zz = attn_z<DT, MDT>(attn_a<DT, MDT>(x, MDT == ATTN_NOMASK ? 0.0f : mk[rb][c], a.inv));
                    z[c] = key <= lim[rb] ? zz : LOSS_NEG_INF;              // behind the clamp
                    tmax = __builtin_fmaxf(tmax, z[c]);
                }
                tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 16));
                tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 32));
                const float mn = __builtin_fmaxf(m[rb], tmax), ref = loss_ref(mn);
                const float alpha = attn_exp(m[rb] - ref);                  // m raw: -inf - ref is -inf, never inf - inf
                m[rb] = mn;
                l[rb] = l[rb] * alpha;
                float p[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    p[c] = attn_exp(z[c] - ref);
                    l[rb] += p[c];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float e[2] = {p[2 * i], p[2 * i + 1]};
                    pf[rb][i] = Ty<DT>::pack(e);
                }
#pragma unroll
                for (int i = 0; i < DB; ++i) acc[rb][i] = acc[rb][i] * alpha;
            }
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                u32x4_t vf;
#if PRE_V_TR
                typedef __attribute__((address_space(3))) i16x4_t* lds_i16x4_ptr;
                const char* p0 = vt + (4 * g + (j >> 2)) * RS + 2 * (16 * db + 4 * (j & 3));
                const i16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(uintptr_t)p0);
                const i16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_i16x4_ptr)(uintptr_t)(p0 + 16 * RS));
                vf = __builtin_bit_cast(u32x4_t, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#else
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c0 = 2 * i, c1 = 2 * i + 1;
                    const int r0 = 16 * (c0 >> 2) + 4 * g + (c0 & 3), r1 = 16 * (c1 >> 2) + 4 * g + (c1 & 3);
                    const uint32_t lo = *(const uint16_t*)(vt + r0 * RS + 2 * (16 * db + j));
                    const uint32_t hi = *(const uint16_t*)(vt + r1 * RS + 2 * (16 * db + j));
                    vf[i] = lo | (hi << 16);
                }
#endif
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) acc[rb][db] = dec_mfma<DT>(vf, pf[rb], acc[rb][db]);
            }
        }
        if (more) store_tile(buf ^ 1, kr, vr);
        __syncthreads();
    }

#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const float sum = dec_sum_groups(l[rb]);
        if (trow[rb] < T) {
            const int64_t o = ((b * T + trow[rb]) * a.H + h) * D + 4 * g;
#pragma unroll
            for (int db = 0; db < DB; ++db) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Ty<DT>::store1(a.out, o + 16 * db + r, acc[rb][db][r] / sum);
            }
            if constexpr (STATS) {
                if (g == 0 && a.stats) {
                    float* st = a.stats + 2 * ((b * a.H + h) * T + trow[rb]);
                    st[0] = m[rb], st[1] = sum;
                }
            }
        }
    }
}

}  // namespace fq
