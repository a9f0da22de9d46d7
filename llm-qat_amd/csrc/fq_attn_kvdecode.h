// fq_attn_kvdecode.h -- the decode attention over a K/V cache held as integer codes: the kernel behind
// include/llmqat_fakequant_attn_kvdecode.h.
//
//   out[b, t, h, :] = softmax(max(rb(rb(q khat^T) inv) + mask, finfo.min), -1) vhat      khat = rope(rb(code_k / t2_k)), vhat = rb(code_v / t2_v)
//
// fq_attn_decode.h's kernel with another operand stage: k and v never exist as 16-bit tensors.  The work split, the softmax step, the wave
// merge, the chunk combine and every guard are that file's own functions (dec_softmax_step, dec_load_mask, dec_finish, dec_combine_kernel,
// fq_shapes.h's split rule); what is new is how the two A operands are made.
//
// K.  The score instruction sums over d in whatever order its two operands share.  Lane (j, g) of a 16-key half tile holds, of key row j,
//     the HB = D / 8 codes d = HB g .. HB g + HB - 1 and their rotary partners D / 2 + HB g ..: two loads of HB codes (16 bytes of int8 or
//     8 bytes of int4 for D = 128), one t2, one position and the cos / sin values of those 2 HB columns.  Element e of the lane (e < HB:
//     the first half, else the second) is k index e & 7 of k-step e >> 3, and q is loaded with the same permutation.  Dequantization,
//     rope_fwd (fq_rope.h's own element pair) and the packing to the dtype happen in registers: nothing crosses lanes, K never meets LDS.
// V.  The wave stages its 32 x D tile in LDS as codes (rows of D or D / 2 bytes, padded by 16) together with (t2, 1 / t2) of the 32 keys.
//     Lane (j, g) reads, for each of its eight keys, the DB = D / 16 codes d = DB j .. DB j + DB - 1 with ONE LDS load and dequantizes
//     them into the A operands of the DB PV instructions: accumulator block db then holds d = DB (4 g + r) + db (dec_col's PERM).  The
//     key order of the PV instruction's k dimension is dec_kernel's.
// Order per tile: this tile's V codes, t2 and mask, the next tile's K codes, t2 and table values (its positions were loaded a tile
//     earlier) and the positions of the tile after that are issued; then the QK instructions, the softmax, the LDS hop, PV, and last the
//     next tile's K operand is built from what has arrived meanwhile.
//
// Dequantization.  code / t2 is the correctly rounded fp32 quotient: Markstein's correction of a reciprocal multiply (fq_device.h's
// div_exact without its two selects: a code is a finite integer and never -0, so neither the infinite numerator nor the negative zero
// it guards exists) where every t2 of the wave's tile lies in div_exact_ok's range, the IEEE division behind a wave-uniform branch
// otherwise.  One rounding to the dtype follows.
//
// VEC: 16- / 8- / 4-byte loads where every base and stride allows them; else byte loads (2-byte for q and the tables) into the same registers.
#pragma once
#include "fq_attn_decode.h"
#include "fq_rope.h"

namespace fq {

struct KvdArgs {
    DecArgs d;            // k, v: the codes; ks, vs: their strides in bytes
    const float* kt2;     // [B, S] by batch stride
    const float* vt2;
    int64_t kt2_bs, vt2_bs;
    const void* cos;      // [P, D] of the dtype, rows contiguous; nullptr: no rotation
    const void* sin;
    const int64_t* pos;   // [B, S] by batch stride (0: one row for all); nullptr: the key index
    int64_t pos_bs, P;
};

template <bool VEC, int NW> __device__ __forceinline__ void kvd_ld(const uint8_t* p, uint32_t (&w)[NW]) {
    static_assert(NW == 1 || NW == 2 || NW == 4, "4, 8 or 16 bytes");
    if constexpr (!VEC) {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    } else if constexpr (NW == 4) {
        const u32x4_t v = *(const u32x4_t*)p;
        w[0] = v[0], w[1] = v[1], w[2] = v[2], w[3] = v[3];
    } else if constexpr (NW == 2) {
        const u32x2_t v = *(const u32x2_t*)p;
        w[0] = v[0], w[1] = v[1];
    } else {
        w[0] = *(const uint32_t*)p;
    }
}
// code i of a little-endian stream of CB-bit two's-complement codes (int4: element 2 k in the low nibble of byte k), as a float
template <int CB> __device__ __forceinline__ float kvd_code(const uint32_t* w, int i) {
    constexpr int PER = 32 / CB;
    return (float)((int32_t)(w[i / PER] << (32 - CB - CB * (i % PER))) >> (32 - CB));
}
// N codes of one key over its divisor: the fp32 quotients; fast: wave-uniform, every divisor of the wave lies in div_exact_ok's range
template <int N> __device__ __forceinline__ void kvd_div(float (&x)[N], float t2, float r, bool fast) {
    if (fast) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float q0 = x[i] * r;
            x[i] = __builtin_fmaf(__builtin_fmaf(-q0, t2, x[i]), r, q0);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = x[i] / t2;
    }
}
__device__ __forceinline__ bool kvd_all(bool p) { return __builtin_amdgcn_ballot_w64(!p) == 0; }

template <int D, int CB> constexpr int kvd_row_bytes() { return D * CB / 8 + 16; }
template <int D, int CB> constexpr int kvd_stage_bytes() { return DEC_TILE * kvd_row_bytes<D, CB>() + DEC_TILE * 8; }
template <int D, int CB> constexpr int kvd_smem_bytes() {
    constexpr int stage = DEC_WAVES * kvd_stage_bytes<D, CB>(), merge = (DEC_WAVES - 1) * 64 * (4 * (D / 16) + 2) * 4;
    return stage > merge ? stage : merge;
}

// the whole workgroup's work under either column map (dec_column); kvd_kernel and the grouped kernel (fq_attn_gqa.h) are this body
template <int DT, int MDT, int D, int CB, bool ROT, bool VEC, bool GQA>
__device__ __forceinline__ void kvd_body(const KvdArgs& ka) {
    static_assert((D == 64 || D == 128) && (CB == 8 || CB == 4), "head sizes and containers served");
    using T = Ty<DT>;
    constexpr int KS = D / 32;                  // k-steps of a score tile
    constexpr int DB = D / 16;                  // 16-column blocks of the output
    constexpr int HB = D / 8;                   // codes of a lane per half of a key row
    constexpr int KW = HB * CB / 32;            // words of those codes
    constexpr int TW = HB / 2;                  // words of HB table values
    constexpr int VB = D * CB / 8;              // bytes of a V row
    constexpr int RS = kvd_row_bytes<D, CB>();
    constexpr int STAGE = kvd_stage_bytes<D, CB>();
    constexpr int LPR = VB / 16;                // lanes of a V row (16 bytes each)
    constexpr int RPI = 64 / LPR;               // V rows of one load instruction
    constexpr int NVI = DEC_TILE / RPI;         // V load instructions of a tile
    constexpr int RBY = DB * CB / 8;            // bytes of a lane's codes of one V key
    constexpr int RW = RBY >= 4 ? RBY / 4 : 1;
    __shared__ __attribute__((aligned(16))) char smem[kvd_smem_bytes<D, CB>()];

    const DecArgs& a = ka.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const DecCol col = dec_column<GQA>(a, j);
    const int64_t b = col.b;
    const int64_t S = a.S, last = S - 1;
    const int64_t t0 = (int64_t)blockIdx.y * a.per;
    const int64_t nt = (S + DEC_TILE - 1) / DEC_TILE;
    const int64_t t1 = t0 + a.per < nt ? t0 + a.per : nt;

    const uint16_t* qp = (const uint16_t*)a.q + b * a.qs[0] + col.h * a.qs[1] + col.t * a.qs[2] + HB * g;
    const uint8_t* kp = (const uint8_t*)a.k + b * a.ks[0] + col.kvh * a.ks[1] + HB * g * CB / 8;
    const uint8_t* vp = (const uint8_t*)a.v + b * a.vs[0] + col.kvh * a.vs[1] + 16 * (lane % LPR);
    const float* kt2 = ka.kt2 + b * ka.kt2_bs;
    const float* vt2 = ka.vt2 + b * ka.vt2_bs;
    const int64_t* pos = ka.pos ? ka.pos + b * ka.pos_bs : nullptr;
    const int64_t mb = MDT == ATTN_NOMASK ? 0 : b * a.mbs + col.t * a.mrs;
    const int vrow = lane / LPR;
    char* stage = smem + wave * STAGE;
    float2* vscale = (float2*)(stage + DEC_TILE * RS);

    u32x4_t qf[KS];                             // q in K's order of d: element e of the lane is d = (e / HB) D / 2 + HB g + e % HB
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const u32x4_t x = dec_ld16<VEC>(qp + (8 * ks / HB) * (D / 2) + 8 * ks % HB);
        qf[ks] = col.live ? x : (u32x4_t){0u, 0u, 0u, 0u};
    }

    struct KRaw {                               // what the K operand of one tile is made of, per 16-key half: [hf]
        uint32_t code[2][2][KW];                // [hf][first / second half of d]
        float t2[2];
        uint32_t tab[2][4][ROT ? TW : 1];       // cos first, cos second, sin first, sin second
        bool in[2];
    };
    // the table rows of a tile's two keys of this lane: -1 where the position lies outside the table (fq_rope.h's rule)
    auto load_pos = [&](int64_t tile, int64_t (&row)[2]) {
        if constexpr (ROT) {
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                int64_t key = tile * DEC_TILE + 16 * hf + j;
                key = key < last ? key : last;
                int64_t p = pos ? pos[key] : key;
                if (p < 0) p += ka.P;
                row[hf] = p >= 0 && p < ka.P ? p : -1;
            }
        }
    };
    auto load_k = [&](int64_t tile, const int64_t (&row)[2], KRaw& r) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            int64_t key = tile * DEC_TILE + 16 * hf + j;
            key = key < last ? key : last;
            const uint8_t* p = kp + key * a.ks[2];
            kvd_ld<VEC>(p, r.code[hf][0]);
            kvd_ld<VEC>(p + D / 2 * CB / 8, r.code[hf][1]);
            r.t2[hf] = kt2[key];
            if constexpr (ROT) {
                r.in[hf] = row[hf] >= 0;
                const int64_t at = (r.in[hf] ? row[hf] : 0) * D + HB * g;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint16_t* tp = (const uint16_t*)(w < 2 ? ka.cos : ka.sin) + at + (w & 1) * (D / 2);
#pragma unroll
                    for (int v = 0; v < TW / 4; ++v) {
                        const u32x4_t x = dec_ld16<VEC>(tp + 8 * v);
                        r.tab[hf][w][4 * v] = x[0], r.tab[hf][w][4 * v + 1] = x[1], r.tab[hf][w][4 * v + 2] = x[2], r.tab[hf][w][4 * v + 3] = x[3];
                    }
                }
            }
        }
    };
    // codes -> rb(code / t2) -> rope_fwd -> the A operands of the tile's score instructions
    auto make_k = [&](const KRaw& r, u32x4_t (&kf)[2 * KS]) {
        const bool fast = kvd_all(div_exact_ok(r.t2[0]) && div_exact_ok(r.t2[1]));
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const float t2 = r.t2[hf], rc = 1.0f / t2;
            float x1[HB], x2[HB];
#pragma unroll
            for (int i = 0; i < HB; ++i) x1[i] = kvd_code<CB>(r.code[hf][0], i), x2[i] = kvd_code<CB>(r.code[hf][1], i);
            kvd_div(x1, t2, rc, fast);
            kvd_div(x2, t2, rc, fast);
            uint32_t kw[HB];                    // word e / 2 of the lane's 2 HB elements
#pragma unroll
            for (int i = 0; i < HB; i += 2) {
                float y1[2] = {x1[i], x1[i + 1]}, y2[2] = {x2[i], x2[i + 1]};
                if constexpr (ROT) {
                    float c1[2], c2[2], s1[2], s2[2];
                    T::unpack(r.tab[hf][0][i / 2], c1);
                    T::unpack(r.tab[hf][1][i / 2], c2);
                    T::unpack(r.tab[hf][2][i / 2], s1);
                    T::unpack(r.tab[hf][3][i / 2], s2);
                    rope_outside<2>(r.in[hf], c1, c2, s1, s2);
                    T::round_dt(y1);
                    T::round_dt(y2);
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const float u1 = y1[e], u2 = y2[e];
                        rope_fwd<DT>(u1, u2, c1[e], c2[e], s1[e], s2[e], y1[e], y2[e]);
                    }
                }
                kw[i / 2] = T::pack(y1);
                kw[HB / 2 + i / 2] = T::pack(y2);
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kf[hf * KS + ks] = (u32x4_t){kw[4 * ks], kw[4 * ks + 1], kw[4 * ks + 2], kw[4 * ks + 3]};
        }
    };

    float m = LOSS_NEG_INF, l = 0.0f;
    f32x4_t acc[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) acc[i] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};

    int64_t tile = t0 + wave;
    if (tile < t1) {
        u32x4_t kf[2 * KS];
        int64_t rown[2] = {0, 0};
        {
            KRaw r;
            load_pos(tile, rown);
            load_k(tile, rown, r);
            load_pos(tile + DEC_WAVES, rown);
            make_k(r, kf);
        }
        for (; tile < t1; tile += DEC_WAVES) {
            // this tile's V codes, divisors and mask; the next tile's K (clamped: a tile past the chunk re-reads in-range rows and is dropped)
            uint32_t vr[NVI][4];
#pragma unroll
            for (int it = 0; it < NVI; ++it) {
                int64_t key = tile * DEC_TILE + it * RPI + vrow;
                key = key < last ? key : last;
                kvd_ld<VEC>(vp + key * a.vs[2], vr[it]);
            }
            int64_t vkey = tile * DEC_TILE + (lane & 31);
            vkey = vkey < last ? vkey : last;
            const float vt = vt2[vkey];
            float mk[8];
            dec_load_mask<MDT>(a.mask, mb, tile, g, last, mk);
            KRaw rn;
            load_k(tile + DEC_WAVES, rown, rn);
            load_pos(tile + 2 * DEC_WAVES, rown);

            f32x4_t sc[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                sc[hf] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) sc[hf] = dec_mfma<DT>(kf[hf * KS + ks], qf[ks], sc[hf]);
            }
            const u32x4_t pf = dec_softmax_step<DT, MDT>(sc, mk, tile, g, S, a.inv, m, l, acc);

            // V through the wave's stage, as codes; lanes l and l + 32 write the same (t2, 1 / t2) of key l
#pragma unroll
            for (int it = 0; it < NVI; ++it) *(u32x4_t*)(stage + (it * RPI + vrow) * RS + 16 * (lane % LPR)) = (u32x4_t){vr[it][0], vr[it][1], vr[it][2], vr[it][3]};
            vscale[lane & 31] = make_float2(vt, 1.0f / vt);
            const bool vfast = kvd_all(div_exact_ok(vt));
            dec_wave_sync();
            uint32_t vw[8][RW];
            float2 vs[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int r = 16 * (c >> 2) + 4 * g + (c & 3);
                const char* p = stage + r * RS + j * RBY;
                if constexpr (RBY == 8) {
                    const u32x2_t x = *(const u32x2_t*)p;
                    vw[c][0] = x[0], vw[c][1] = x[1];
                } else if constexpr (RBY == 4) {
                    vw[c][0] = *(const uint32_t*)p;
                } else {
                    vw[c][0] = *(const uint16_t*)p;
                }
                vs[c] = vscale[r];
            }
            float vx[8][DB];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
#pragma unroll
                for (int db = 0; db < DB; ++db) vx[c][db] = kvd_code<CB>(vw[c], db);
                kvd_div(vx[c], vs[c].x, vs[c].y, vfast);
            }
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                u32x4_t vf;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float e[2] = {vx[2 * i][db], vx[2 * i + 1][db]};
                    vf[i] = T::pack(e);
                }
                acc[db] = dec_mfma<DT>(vf, pf, acc[db]);
            }
            dec_wave_sync();
            make_k(rn, kf);
        }
    }
    dec_finish<DT, D, true>(smem, m, l, acc, a.out, a.ws, a.H, a.T, a.nsplit, col);
}

template <int DT, int MDT, int D, int CB, bool ROT, bool VEC>
__global__ __launch_bounds__(DEC_WAVES * 64) void kvd_kernel(KvdArgs ka) { kvd_body<DT, MDT, D, CB, ROT, VEC, false>(ka); }

}  // namespace fq
