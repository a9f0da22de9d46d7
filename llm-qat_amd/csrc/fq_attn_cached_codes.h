// fq_attn_cached_codes.h -- the decode attention over an in-place K/V cache of integer codes with device lengths: the
// kernel behind include/llmqat_fakequant_attn_cached_codes.h.
//
// Section 35's call (fq_attn_cached.h) on section 33's operands (fq_attn_kvdecode.h).  The caches hold the codes, [B, Hkv, Smax, D] int8 or
// [B, Hkv, Smax, D / 2] packed int4, beside one fp32 divisor per token, [B, Smax] for K and for V; batch row b holds len_b = cache_lens[b]
// valid keys and the call brings T <= 16 new ones as codes and divisors.  ONE launch appends them at len_b .. len_b + T - 1 and attends:
// query row t sees the keys start_b <= s <= len_b + t, khat = rope(rb(code / t2)) at position s - start_b and vhat = rb(code / t2), made in
// registers.  The 16-bit k and v never exist, and neither does a positions tensor: the table row is derived from the key index.
//
// Work split: cac_body's.  Grid (B Hkv NP, nsplit) with dec_column<true>'s packs, nsplit from Smax alone; a workgroup cuts ITS batch row's
// tiles (len_b + T keys, less the whole tiles in front of start_b) into min(nsplit, tiles / DEC_MIN_TILES) chunks and takes chunk
// blockIdx.y; a chunk past the last writes the neutral partial, and dec_finish / gqa_combine_kernel merge in wave and chunk order.
//
// K: kvd_body's register path (two loads of HB codes of key row j, one t2, the table values of 2 HB columns; ccc_make_k dequantizes,
//    rotates and packs).  Whether a key's codes and t2 come from the cache (s < len_b) or from the new tensors is chosen per lane in the
//    address; the table row s - start_b needs no load, so the pipeline is one stage shorter than kvd_body's (no positions in flight).
// V: the wave's 32-key tile is staged in LDS as codes beside (t2, 1 / t2), each row from the cache or the new tensor by the same rule;
//    ccc_pv reads it back and feeds the PV instructions.
// Append: no workgroup reads a row of a cache at or past len_b, and only such rows are written: nothing is ordered.  The workgroup of pack
//    0 and chunk 0 copies the T code rows of its (b, kvh) for K and V, 16 bytes a store on the VEC path and bytes otherwise; where
//    kvh == 0 it also writes the 2 T divisors of the batch row.  Plain vector stores.
//
// Guards: fq_attn_cached.h's.  A negative length counts as 0, one above Smax as Smax, a start is brought into [0, len_b]; a new row that
// would land at or past Smax is not stored and still takes part.  Every cache row formed is below len_b <= Smax, every new row within
// [0, T), every table row within [0, P) (a position at or past P: NaN tables, fq_rope.h's rule; the host checks P >= Smax).
#pragma once
#include "fq_attn_gqa.h"

namespace fq {

struct CccArgs {
    DecArgs d;                          // q, out, ws, qs, H, T, nsplit, inv, Hkv, G, HP, NP as the grouped decode launch's; S: Smax
    const uint8_t *kn, *vn;             // the new codes [B, Hkv, T, D CB / 8] by byte strides
    uint8_t *kc, *vc;                   // the code caches [B, Hkv, Smax, D CB / 8] by byte strides
    int64_t kns[3], vns[3], kcs[3], vcs[3];
    const float *kt2n, *vt2n;           // the new divisors [B, T] by batch stride
    float *kt2c, *vt2c;                 // the divisor caches [B, Smax] by batch stride
    int64_t kt2n_bs, vt2n_bs, kt2c_bs, vt2c_bs;
    const void *cos, *sin;              // [P, D] of the dtype, rows contiguous; nullptr: no rotation
    int64_t P;
    const int* lens;                    // [B]
    const int* starts;                  // [B] or nullptr
};

// ---- kvd_body's two operand stages as functions.  That body keeps them inline (lifting them out of it moved its register allocation, and
// the existing units' code stays as it was measured); the arithmetic below is the same, statement for statement -----------------------------
// what the K operand of one tile is made of, per 16-key half: [hf]
template <int D, int CB, bool ROT> struct CccRaw {
    uint32_t code[2][2][D / 8 * CB / 32];       // [hf][first / second half of d]
    float t2[2];
    uint32_t tab[2][4][ROT ? D / 16 : 1];       // cos first, cos second, sin first, sin second
    bool in[2];
};
// codes -> rb(code / t2) -> rope_fwd -> the A operands of the tile's score instructions
template <int DT, int D, int CB, bool ROT> __device__ __forceinline__ void ccc_make_k(const CccRaw<D, CB, ROT>& r, u32x4_t (&kf)[2 * (D / 32)]) {
    using T = Ty<DT>;
    constexpr int KS = D / 32, HB = D / 8;
    const bool fast = kvd_all(div_exact_ok(r.t2[0]) && div_exact_ok(r.t2[1]));
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
        const float t2 = r.t2[hf], rc = 1.0f / t2;
        float x1[HB], x2[HB];
#pragma unroll
        for (int i = 0; i < HB; ++i) x1[i] = kvd_code<CB>(r.code[hf][0], i), x2[i] = kvd_code<CB>(r.code[hf][1], i);
        kvd_div(x1, t2, rc, fast);
        kvd_div(x2, t2, rc, fast);
        uint32_t kw[HB];                        // word e / 2 of the lane's 2 HB elements
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
}
// the wave's staged V tile (codes beside (t2, 1 / t2)) -> the A operands of the DB PV instructions, accumulated with pf into acc
template <int DT, int D, int CB>
__device__ __forceinline__ void ccc_pv(const char* stage, const float2* vscale, bool vfast, int j, int g, u32x4_t pf, f32x4_t (&acc)[D / 16]) {
    using T = Ty<DT>;
    constexpr int DB = D / 16, RS = kvd_row_bytes<D, CB>();
    constexpr int RBY = DB * CB / 8;            // bytes of a lane's codes of one V key
    constexpr int RW = RBY >= 4 ? RBY / 4 : 1;
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
}

// the T new code rows of k and v of (b, kvh) into rows len .. of the caches and, lead, the batch row's 2 T divisors; the whole workgroup calls
template <int D, int CB, bool VEC> __device__ __forceinline__ void ccc_append(const CccArgs& ca, int64_t b, int64_t kvh, int64_t len, bool lead) {
    constexpr int PPR = D * CB / 128;                       // 16-byte pieces of a code row
    const int T = (int)ca.d.T, n = 2 * T * PPR;
    for (int i = threadIdx.x; i < n; i += DEC_WAVES * 64) {
        const bool isv = i >= T * PPR;
        const int rem = isv ? i - T * PPR : i, t = rem / PPR, piece = rem % PPR;
        if (len + t >= ca.d.S) continue;                    // past the cache: not stored
        const int64_t* ns = isv ? ca.vns : ca.kns;
        const int64_t* cs = isv ? ca.vcs : ca.kcs;
        const uint8_t* src = (isv ? ca.vn : ca.kn) + b * ns[0] + kvh * ns[1] + t * ns[2] + 16 * piece;
        uint8_t* dst = (isv ? ca.vc : ca.kc) + b * cs[0] + kvh * cs[1] + (len + t) * cs[2] + 16 * piece;
        if constexpr (VEC) {
            *(u32x4_t*)dst = *(const u32x4_t*)src;
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) dst[e] = src[e];
        }
    }
    if (lead && (int)threadIdx.x < 2 * T) {
        const bool isv = (int)threadIdx.x >= T;
        const int t = isv ? threadIdx.x - T : threadIdx.x;
        if (len + t < ca.d.S) {
            if (isv) ca.vt2c[b * ca.vt2c_bs + len + t] = ca.vt2n[b * ca.vt2n_bs + t];
            else ca.kt2c[b * ca.kt2c_bs + len + t] = ca.kt2n[b * ca.kt2n_bs + t];
        }
    }
}

template <int DT, int D, int CB, bool ROT, bool VEC> __device__ __forceinline__ void ccc_body(const CccArgs& ca) {
    static_assert((D == 64 || D == 128) && (CB == 8 || CB == 4), "head sizes and containers served");
    const DecArgs& a = ca.d;
    constexpr int KS = D / 32, DB = D / 16, HB = D / 8, TW = HB / 2;      // kvd_body's constants
    constexpr int VB = D * CB / 8;
    constexpr int RS = kvd_row_bytes<D, CB>();
    constexpr int STAGE = kvd_stage_bytes<D, CB>();
    constexpr int LPR = VB / 16, RPI = 64 / LPR, NVI = DEC_TILE / RPI;
    using KRaw = CccRaw<D, CB, ROT>;
    __shared__ __attribute__((aligned(16))) char smem[kvd_smem_bytes<D, CB>()];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const DecCol col = dec_column<true>(a, j);
    const int64_t b = col.b;

    // the batch row's own geometry, from the device lengths: cac_body's
    int64_t len = ca.lens[b];
    len = len < 0 ? 0 : len > a.S ? a.S : len;
    int64_t start = ca.starts ? ca.starts[b] : 0;
    start = start < 0 ? 0 : start > len ? len : start;
    const int64_t total = len + a.T, last = total - 1;
    const int64_t tlo = start / DEC_TILE, ntiles = (total + DEC_TILE - 1) / DEC_TILE - tlo;     // >= 1: key `last` is behind start
    int64_t n = ntiles / DEC_MIN_TILES;
    n = n < 1 ? 1 : n < a.nsplit ? n : a.nsplit;
    const int64_t per = (ntiles + n - 1) / n;
    const int64_t t0 = tlo + (int64_t)blockIdx.y * per;
    const int64_t t1 = t0 + per < tlo + ntiles ? t0 + per : tlo + ntiles;      // t0 >= t1: an empty chunk

    if (blockIdx.y == 0 && blockIdx.x % a.NP == 0) ccc_append<D, CB, VEC>(ca, b, col.kvh, len, col.kvh == 0);

    const uint16_t* qp = (const uint16_t*)a.q + b * a.qs[0] + col.h * a.qs[1] + col.t * a.qs[2] + HB * g;
    const uint8_t* kcp = ca.kc + b * ca.kcs[0] + col.kvh * ca.kcs[1] + HB * g * CB / 8;
    const uint8_t* knp = ca.kn + b * ca.kns[0] + col.kvh * ca.kns[1] + HB * g * CB / 8;
    const uint8_t* vcp = ca.vc + b * ca.vcs[0] + col.kvh * ca.vcs[1] + 16 * (lane % LPR);
    const uint8_t* vnp = ca.vn + b * ca.vns[0] + col.kvh * ca.vns[1] + 16 * (lane % LPR);
    const float* kt2c = ca.kt2c + b * ca.kt2c_bs;
    const float* kt2n = ca.kt2n + b * ca.kt2n_bs;
    const float* vt2c = ca.vt2c + b * ca.vt2c_bs;
    const float* vt2n = ca.vt2n + b * ca.vt2n_bs;
    const int vrow = lane / LPR;
    char* stage = smem + wave * STAGE;
    float2* vscale = (float2*)(stage + DEC_TILE * RS);
    const int64_t seen = len + col.t + 1;                   // the column's keys end here

    u32x4_t qf[KS];                                         // q in K's order of d, as kvd_body
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const u32x4_t x = dec_ld16<VEC>(qp + (8 * ks / HB) * (D / 2) + 8 * ks % HB);
        qf[ks] = col.live ? x : (u32x4_t){0u, 0u, 0u, 0u};
    }

    // what the K operand of a tile is made of.  A key past the last re-reads the last; below len the cache, from there the new tensors;
    // the table row is the key's position s - start (a key in front of start is unseen: row 0 stands in)
    auto load_k = [&](int64_t tile, KRaw& r) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            int64_t key = tile * DEC_TILE + 16 * hf + j;
            key = key < last ? key : last;
            const bool old = key < len;
            const uint8_t* p = old ? kcp + key * ca.kcs[2] : knp + (key - len) * ca.kns[2];
            kvd_ld<VEC>(p, r.code[hf][0]);
            kvd_ld<VEC>(p + D / 2 * CB / 8, r.code[hf][1]);
            r.t2[hf] = *(old ? kt2c + key : kt2n + (key - len));
            if constexpr (ROT) {
                const int64_t row = key < start ? 0 : key - start;
                r.in[hf] = row < ca.P;
                const int64_t at = (r.in[hf] ? row : 0) * D + HB * g;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint16_t* tp = (const uint16_t*)(w < 2 ? ca.cos : ca.sin) + at + (w & 1) * (D / 2);
#pragma unroll
                    for (int v = 0; v < TW / 4; ++v) {
                        const u32x4_t x = dec_ld16<VEC>(tp + 8 * v);
                        r.tab[hf][w][4 * v] = x[0], r.tab[hf][w][4 * v + 1] = x[1], r.tab[hf][w][4 * v + 2] = x[2], r.tab[hf][w][4 * v + 3] = x[3];
                    }
                }
            }
        }
    };

    float m = LOSS_NEG_INF, l = 0.0f;
    f32x4_t acc[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) acc[i] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};

    int64_t tile = t0 + wave;
    if (tile < t1) {
        u32x4_t kf[2 * KS];
        {
            KRaw r;
            load_k(tile, r);
            ccc_make_k<DT, D, CB, ROT>(r, kf);
        }
        for (; tile < t1; tile += DEC_WAVES) {
            // this tile's V codes and divisors, the next tile's K (a tile past the chunk re-reads in-range rows and is dropped)
            uint32_t vr[NVI][4];
#pragma unroll
            for (int it = 0; it < NVI; ++it) {
                int64_t key = tile * DEC_TILE + it * RPI + vrow;
                key = key < last ? key : last;
                kvd_ld<VEC>(key < len ? vcp + key * ca.vcs[2] : vnp + (key - len) * ca.vns[2], vr[it]);
            }
            int64_t vkey = tile * DEC_TILE + (lane & 31);
            vkey = vkey < last ? vkey : last;
            const float vt = *(vkey < len ? vt2c + vkey : vt2n + (vkey - len));
            float mk[8];
            dec_load_mask<ATTN_NOMASK>(nullptr, 0, tile, g, last, mk);
            KRaw rn;
            load_k(tile + DEC_WAVES, rn);

            f32x4_t sc[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                sc[hf] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) sc[hf] = dec_mfma<DT>(kf[hf * KS + ks], qf[ks], sc[hf]);
            }
            const u32x4_t pf = dec_softmax_step<DT, ATTN_NOMASK, DB, true>(sc, mk, tile, g, seen, a.inv, m, l, acc, start);

            // V through the wave's stage, as codes; lanes l and l + 32 write the same (t2, 1 / t2) of key l
#pragma unroll
            for (int it = 0; it < NVI; ++it) *(u32x4_t*)(stage + (it * RPI + vrow) * RS + 16 * (lane % LPR)) = (u32x4_t){vr[it][0], vr[it][1], vr[it][2], vr[it][3]};
            vscale[lane & 31] = make_float2(vt, 1.0f / vt);
            const bool vfast = kvd_all(div_exact_ok(vt));
            dec_wave_sync();
            ccc_pv<DT, D, CB>(stage, vscale, vfast, j, g, pf, acc);
            dec_wave_sync();
            ccc_make_k<DT, D, CB, ROT>(rn, kf);
        }
    }
    dec_finish<DT, D, true>(smem, m, l, acc, a.out, a.ws, a.H, a.T, a.nsplit, col);
}

template <int DT, int D, int CB, bool ROT, bool VEC>
__global__ __launch_bounds__(DEC_WAVES * 64) void ccc_kernel(CccArgs ca) { ccc_body<DT, D, CB, ROT, VEC>(ca); }

}  // namespace fq
