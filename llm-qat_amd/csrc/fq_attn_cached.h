// fq_attn_cached.h -- the decode attention over an in-place K/V cache with device lengths: the kernel behind
// include/llmqat_fakequant_attn_cached.h.
//
// k_cache, v_cache [B, Hkv, Smax, D] are preallocated; batch row b holds len_b = cache_lens[b] valid keys and the call brings T <= 16 new
// ones, k_new, v_new [B, Hkv, T, D].  ONE launch appends the new rows at len_b .. len_b + T - 1 and attends: query row t of batch row b
// sees the keys start_b <= s <= len_b + t of the updated cache.  The lengths are read here, on the device; the host never sees them.
//
// Where a key comes from.  Key s < len_b is row s of the cache, key len_b <= s < len_b + T is row s - len_b of k_new / v_new: the choice
// is made per lane in the address of the K operand loads and of the V stage loads, which are addressed per lane anyway.  So NO workgroup
// of the launch reads a cache row at or past len_b, and the only writes to the caches are rows at or past len_b: the append has nothing
// to be ordered against, inside the launch or between its workgroups.  Exactly one workgroup per (batch, K/V head), the one of pack 0 and
// chunk 0, copies the T new rows of k and v in, with 16-byte stores on the VEC path.
//
// Work split.  The launch shape is static: grid (B Hkv NP, nsplit) with the grouped decode kernel's packs (dec_column<true>: HP query
// heads of a K/V head share the 16 columns) and nsplit = dec_nsplit(B Hkv NP, Smax, cus), whatever the lengths are.  A workgroup cuts ITS
// batch row's tiles -- those of len_b + T keys, less the whole tiles in front of start_b -- into min(nsplit, tiles / DEC_MIN_TILES)
// chunks (at least one) and takes chunk blockIdx.y; a chunk past the last writes the neutral partial (m, l, acc) = (-inf, 0, 0), which
// dec_merge and dec_combine absorb through loss_ref.  A short row in a batch of long ones is therefore still spread over as many
// workgroups as it can fill, and a long one is not cut by the shortest.
//
// Seen / unseen is an index comparison behind the score (dec_softmax_step<.., LOW>): start_b <= key <= len_b + t, per column; no mask is
// read and the chain is the no-mask one (both roundings, no clamp).  Key len_b + t is always seen, so no column's sum is 0.
//
// Guards.  The kernel trusts no int32: a negative length counts as 0, one above Smax as Smax, a start is brought into [0, len_b].  A
// new row that would land at or past Smax is not stored and still takes part, straight from k_new.  Every cache row index formed is
// below len_b <= Smax and every new row index within [0, T): no address outside the tensors exists, whatever the lengths hold.
// VEC: 16-byte loads and stores where every base and stride of q, k_new, v_new and both caches allows; else 2-byte ones.
#pragma once
#include "fq_attn_gqa.h"

namespace fq {

struct CacArgs {
    DecArgs d;               // q, out, ws, qs, H, T, nsplit, inv, Hkv, G, HP, NP as the grouped decode launch's; S: Smax; k, v, mask, per unused
    const void *kn, *vn;     // k_new, v_new [B, Hkv, T, D] by strides
    void *kc, *vc;           // the caches [B, Hkv, Smax, D] by strides
    int64_t kns[3], vns[3], kcs[3], vcs[3];
    const int* lens;         // [B]
    const int* starts;       // [B] or nullptr
};

// the T new rows of k and v of (b, kvh) into rows len .. of the caches; the whole workgroup calls
template <int D, bool VEC> __device__ __forceinline__ void cac_append(const CacArgs& ca, int64_t b, int64_t kvh, int64_t len) {
    constexpr int PPR = D / 8;                              // 16-byte pieces of a row
    const int T = (int)ca.d.T, n = 2 * T * PPR;
    for (int i = threadIdx.x; i < n; i += DEC_WAVES * 64) {
        const bool isv = i >= T * PPR;
        const int rem = isv ? i - T * PPR : i, t = rem / PPR, piece = rem % PPR;
        if (len + t >= ca.d.S) continue;                    // past the cache: not stored
        const int64_t* ns = isv ? ca.vns : ca.kns;
        const int64_t* cs = isv ? ca.vcs : ca.kcs;
        const uint16_t* src = (const uint16_t*)(isv ? ca.vn : ca.kn) + b * ns[0] + kvh * ns[1] + t * ns[2] + 8 * piece;
        uint16_t* dst = (uint16_t*)(isv ? ca.vc : ca.kc) + b * cs[0] + kvh * cs[1] + (len + t) * cs[2] + 8 * piece;
        if constexpr (VEC) {
            *(u32x4_t*)dst = *(const u32x4_t*)src;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[e] = src[e];
        }
    }
}

template <int DT, int D, bool VEC> __device__ __forceinline__ void cac_body(const CacArgs& ca) {
    static_assert(D == 64 || D == 128, "head sizes served");
    const DecArgs& a = ca.d;
    constexpr int KS = D / 32, DB = D / 16;                 // dec_body's constants
    constexpr int RS = dec_row_bytes<D>();
    constexpr int STAGE = dec_stage_bytes<D>();
    constexpr int LPR = D / 8, RPI = 64 / LPR, NVI = DEC_TILE / RPI;
    constexpr int PART = 4 * DB + 2;
    static_assert((DEC_WAVES - 1) * 64 * PART * 4 <= DEC_WAVES * STAGE, "the merge fits the staging area");
    __shared__ __attribute__((aligned(16))) char smem[DEC_WAVES * STAGE];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const DecCol col = dec_column<true>(a, j);
    const int64_t b = col.b;

    // the batch row's own geometry, from the device lengths
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

    if (blockIdx.y == 0 && blockIdx.x % a.NP == 0) cac_append<D, VEC>(ca, b, col.kvh, len);

    const uint16_t* qp = (const uint16_t*)a.q + b * a.qs[0] + col.h * a.qs[1] + col.t * a.qs[2] + 8 * g;
    const uint16_t* kcp = (const uint16_t*)ca.kc + b * ca.kcs[0] + col.kvh * ca.kcs[1] + 8 * g;
    const uint16_t* knp = (const uint16_t*)ca.kn + b * ca.kns[0] + col.kvh * ca.kns[1] + 8 * g;
    const uint16_t* vcp = (const uint16_t*)ca.vc + b * ca.vcs[0] + col.kvh * ca.vcs[1] + 8 * (lane % LPR);
    const uint16_t* vnp = (const uint16_t*)ca.vn + b * ca.vns[0] + col.kvh * ca.vns[1] + 8 * (lane % LPR);
    const int vrow = lane / LPR;
    char* stage = smem + wave * STAGE;
    const int64_t seen = len + col.t + 1;                   // the column's keys end here

    u32x4_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const u32x4_t x = dec_ld16<VEC>(qp + 32 * ks);
        qf[ks] = col.live ? x : (u32x4_t){0u, 0u, 0u, 0u};
    }

    // a key's row: the cache below len, the new tensor from there (a key past the last re-reads the last)
    auto row_of = [&](int64_t key, const uint16_t* cache, int64_t cs, const uint16_t* fresh, int64_t ns) {
        key = key < last ? key : last;
        return key < len ? cache + key * cs : fresh + (key - len) * ns;
    };
    auto load_k = [&](int64_t tile, u32x4_t(&kr)[2 * KS]) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const uint16_t* p = row_of(tile * DEC_TILE + 16 * hf + j, kcp, ca.kcs[2], knp, ca.kns[2]);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) kr[hf * KS + ks] = dec_ld16<VEC>(p + 32 * ks);
        }
    };

    float m = LOSS_NEG_INF, l = 0.0f;
    f32x4_t acc[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) acc[i] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};

    int64_t tile = t0 + wave;
    if (tile < t1) {
        u32x4_t kr[2 * KS];
        load_k(tile, kr);
        for (; tile < t1; tile += DEC_WAVES) {
            u32x4_t vr[NVI];
#pragma unroll
            for (int it = 0; it < NVI; ++it) vr[it] = dec_ld16<VEC>(row_of(tile * DEC_TILE + it * RPI + vrow, vcp, ca.vcs[2], vnp, ca.vns[2]));
            float mk[8];
            dec_load_mask<ATTN_NOMASK>(nullptr, 0, tile, g, last, mk);
            u32x4_t kn[2 * KS];
            load_k(tile + DEC_WAVES, kn);

            f32x4_t sc[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                sc[hf] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) sc[hf] = dec_mfma<DT>(kr[hf * KS + ks], qf[ks], sc[hf]);
            }
            const u32x4_t pf = dec_softmax_step<DT, ATTN_NOMASK, DB, true>(sc, mk, tile, g, seen, a.inv, m, l, acc, start);

            // V through the wave's stage, as dec_body
#pragma unroll
            for (int it = 0; it < NVI; ++it) *(u32x4_t*)(stage + (it * RPI + vrow) * RS + 16 * (lane % LPR)) = vr[it];
            dec_wave_sync();
#pragma unroll
            for (int db = 0; db < DB; ++db) {
                u32x4_t vf;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c0 = 2 * i, c1 = 2 * i + 1;
                    const int r0 = 16 * (c0 >> 2) + 4 * g + (c0 & 3), r1 = 16 * (c1 >> 2) + 4 * g + (c1 & 3);
                    const uint32_t lo = *(const uint16_t*)(stage + r0 * RS + 2 * (16 * db + j));
                    const uint32_t hi = *(const uint16_t*)(stage + r1 * RS + 2 * (16 * db + j));
                    vf[i] = lo | (hi << 16);
                }
                acc[db] = dec_mfma<DT>(vf, pf, acc[db]);
            }
            dec_wave_sync();
#pragma unroll
            for (int i = 0; i < 2 * KS; ++i) kr[i] = kn[i];
        }
    }

    dec_finish<DT, D, false>(smem, m, l, acc, a.out, a.ws, a.H, a.T, a.nsplit, col);
}

template <int DT, int D, bool VEC> __global__ __launch_bounds__(DEC_WAVES * 64) void cac_kernel(CacArgs ca) { cac_body<DT, D, VEC>(ca); }

}  // namespace fq
