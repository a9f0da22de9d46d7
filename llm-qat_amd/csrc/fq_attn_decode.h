// fq_attn_decode.h -- the fused decode attention: the kernels behind include/llmqat_fakequant_attn_decode.h.
//
//   out[b, t, h, :] = softmax(max(rb(rb(q k^T) inv) + mask, finfo.min), -1) v        for T <= 16 query rows against S keys
//
// as ONE stream over K and V: no [B, H, T, S] tensor exists in any precision.  Section 29's chain with the two products around it, the
// per-element roundings by that section's own device functions (attn_a, attn_z, attn_exp); the softmax is online (a running maximum and
// sum per query row), the unnormalised exponentials are rounded to the dtype as the second product's operand, and the division by the
// sum happens once, in fp32, in front of the one output rounding.
//
// Work split.  Grid (B * H, nsplit).  A workgroup of DEC_WAVES waves owns tiles [split * per, (split + 1) * per) of DEC_TILE keys; wave w
// takes tiles w, w + 4, ... of the chunk and keeps (m, l) per query row and an fp32 [16, D] accumulator in registers.  The waves' partials
// are merged by wave 0 through LDS in wave order; with one chunk it divides and writes out, with more it writes (m, l, acc) of the T real
// rows in fp32 to the workspace and dec_combine_kernel merges the chunks in chunk order.  No atomics.
//
// Data movement (v_mfma_f32_16x16x32_{bf16,f16}; lane = 16 g + j).
//   scores   S^T = K q^T.  A = 16 keys of K: lane (j, g) loads the 16 bytes of key row j at d = 32 ks + 8 g straight from global memory
//            (one instruction: 16 rows x 64 bytes).  B = q: lane (j, g) holds q[t = j, 32 ks + 8 g .. + 8], rows >= T zero.  The result
//            registers hold keys 4 g + r (r = 0 .. 3) of query row j.
//   P        two consecutive 16-key tiles give lane (j, g) eight keys of query row j: 4 g + r and 16 + 4 g + r.  That is a B operand of
//            the PV instruction under the k order  k = 8 g + c  <->  key (c < 4 ? 4 g + c : 16 + 4 g + c - 4), which the A operand only
//            has to share.  P never leaves registers.
//   V        A = V^T, 16 columns of d per instruction: lane (j, g) needs V[key(g, c), 16 db + j] for c = 0 .. 7, a transpose.  The wave
//            stages its 32 x D tile in LDS with 16-byte row loads and stores (rows padded by 16 bytes: the four lane groups then read four
//            different bank ranges) and reads it back in that key order with 2-byte reads.  The result registers hold out^T: d = 16 db +
//            4 g + r of query row j, so the per-row factors of the online softmax are the lane's own.
//   order    per tile: V loads of this tile and K loads of the next are issued, then the QK instructions, the softmax, the LDS hop, PV.
//
// Guards.  A key past S clamps its row index on every load (K, V, mask) and is -inf BEHIND the clamp at finfo.min (section 29's trap 2).
// The reference point of a maximum of -inf is 0 (loss_ref) and the old maximum enters exp() raw, so -inf never meets +inf.  A NaN or
// +inf score makes its row's sum NaN and nothing else: the matrix instructions keep query rows in separate columns.  64-bit indices.
// VEC: 16-byte global loads where every base and stride allows them; else 2-byte loads that fill the same registers.
#pragma once
#include "fq_attn_softmax.h"

namespace fq {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

struct DecArgs {
    const void* q;       // [B, H, T, D] by strides (batch, head, token; last stride 1)
    const void* k;       // [B, H, S, D] likewise
    const void* v;
    const void* mask;    // [B, 1, T, S] by (batch, row) stride, or nullptr
    void* out;           // [B, T, H, D] contiguous
    float* ws;           // [B * H, nsplit, T, D + 2]: (m, l, acc) per real query row; nullptr where nsplit == 1
    int64_t qs[3], ks[3], vs[3];
    int64_t mbs, mrs;
    int64_t H, T, S;
    int64_t per;         // tiles of a chunk
    int nsplit;
    float inv;
    int64_t Hkv, G, HP, NP;      // the grouped launch (fq_attn_gqa.h) alone: K/V heads, query heads of one, heads of a pack, packs of a K/V head
};

// What column j of the two matrix instructions stands for in workgroup blockIdx.x.  One head a workgroup (!GQA): token j of head
// blockIdx.x % H.  Grouped: the workgroup is (batch, K/V head, pack) and column j is token j % T of the pack's
// query head j / T.  A dead column (a row >= T, a head past the group) has zero q, a live column's addresses and stores nothing.
struct DecCol {
    int64_t b, h, kvh;   // batch, query head, K/V head
    int t;               // the token whose addresses the lane uses
    bool live;
    int64_t wrow;        // the column's row of the workspace [gridDim.x, nsplit, columns, D + 2]
};
template <bool GQA> __device__ __forceinline__ DecCol dec_column(const DecArgs& a, int j) {
    DecCol c;
    const int64_t x = blockIdx.x;
    const int T = (int)a.T;
    if constexpr (!GQA) {
        c.b = x / a.H, c.h = x % a.H, c.kvh = c.h;
        c.live = j < T;
        c.t = c.live ? j : T - 1;
        c.wrow = (x * a.nsplit + blockIdx.y) * T + j;
    } else {
        const int64_t per = a.Hkv * a.NP, r = x % per;
        const int hl = (int)(r % a.NP) * (int)a.HP + j / T;      // the head within its group
        c.b = x / per, c.kvh = r / a.NP;
        c.live = j < (int)a.HP * T && hl < (int)a.G;
        c.h = c.kvh * a.G + (c.live ? hl : 0);
        c.t = j % T;
        c.wrow = (x * a.nsplit + blockIdx.y) * (a.HP * T) + j;
    }
    return c;
}

template <bool VEC> __device__ __forceinline__ u32x4_t dec_ld16(const uint16_t* p) {
    if constexpr (VEC) {
        return *(const u32x4_t*)p;
    } else {
        u32x4_t r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (uint32_t)p[2 * i] | ((uint32_t)p[2 * i + 1] << 16);
        return r;
    }
}
template <int DT> __device__ __forceinline__ f32x4_t dec_mfma(u32x4_t a, u32x4_t b, f32x4_t c) {
    if constexpr (DT == BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
// LDS accesses of one wave complete in order; this keeps the compiler from moving them across
__device__ __forceinline__ void dec_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the sum over the four lane groups that share a query row (a + b is commutative bit for bit: every lane gets the same bits)
__device__ __forceinline__ float dec_sum_groups(float x) {
    x += __shfl_xor(x, 16);
    return x + __shfl_xor(x, 32);
}
// one more partial (m1, l1, acc1) into (m, l, acc): the online softmax's merge, -inf safe
template <int N> __device__ __forceinline__ void dec_merge(float& m, float& l, f32x4_t (&acc)[N], float m1, float l1, const f32x4_t (&acc1)[N]) {
    const float mn = __builtin_fmaxf(m, m1), ref = loss_ref(mn);
    const float a0 = attn_exp(m - ref), a1 = attn_exp(m1 - ref);
    m = mn;
    l = l * a0 + l1 * a1;
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = acc[i] * a0 + acc1[i] * a1;
}

template <int D> constexpr int dec_row_bytes() { return 2 * D + 16; }
template <int D> constexpr int dec_stage_bytes() { return DEC_TILE * dec_row_bytes<D>(); }

// ---- the stages that dec_kernel and the codes-cache kernel (fq_attn_kvdecode.h) share -----------------------------------------------------
// the online softmax's step over one tile: sc holds the scores of the lane's eight keys (4 g + r of both halves) of query row j, mk their
// mask values.  (m, l) and the accumulator move to the new maximum; -> the rounded exponentials as the PV instruction's B operand.
// S may differ between query rows (lanes of another j); LOW (the in-place cache kernel, fq_attn_cached.h): keys below lo are unseen too
template <int DT, int MDT, int DB, bool LOW = false>
__device__ __forceinline__ u32x4_t dec_softmax_step(const f32x4_t (&sc)[2], const float (&mk)[8], int64_t tile, int g, int64_t S, float inv, float& m,
                                                    float& l, f32x4_t (&acc)[DB], int64_t lo = 0) {
    float z[8];
    float tmax = LOSS_NEG_INF;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int64_t key = tile * DEC_TILE + 16 * (c >> 2) + 4 * g + (c & 3);
        const float x = Ty<DT>::rb(sc[c >> 2][c & 3]);      // the first product's own rounding
        const float zz = attn_z<DT, MDT>(attn_a<DT, MDT>(x, mk[c], inv));
        z[c] = key < S && (!LOW || key >= lo) ? zz : LOSS_NEG_INF;      // behind the clamp
        tmax = __builtin_fmaxf(tmax, z[c]);
    }
    tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 16));
    tmax = __builtin_fmaxf(tmax, __shfl_xor(tmax, 32));
    const float mn = __builtin_fmaxf(m, tmax), ref = loss_ref(mn);
    const float alpha = attn_exp(m - ref);                  // m raw: -inf - ref is -inf, never inf - inf
    m = mn;
    l = l * alpha;
    float p[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        p[c] = attn_exp(z[c] - ref);
        l += p[c];
    }
    u32x4_t pf;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float e[2] = {p[2 * i], p[2 * i + 1]};
        pf[i] = Ty<DT>::pack(e);
    }
#pragma unroll
    for (int i = 0; i < DB; ++i) acc[i] = acc[i] * alpha;
    return pf;
}

// the mask values of the lane's eight keys of a tile (0 without a mask); a key past S re-reads the last
template <int MDT> __device__ __forceinline__ void dec_load_mask(const void* mask, int64_t mb, int64_t tile, int g, int64_t last, float (&mk)[8]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        mk[c] = 0.0f;
        if constexpr (MDT != ATTN_NOMASK) {
            int64_t key = tile * DEC_TILE + 16 * (c >> 2) + 4 * g + (c & 3);
            key = key < last ? key : last;
            mk[c] = Ty<MDT>::load1(mask, mb + key);
        }
    }
}

// the column of `out` that register r of accumulator block db holds in lane group g.  The matrix instruction leaves row 4 g + r of block
// db there; which d that row stands for is the A operand's choice: 16 db + row (dec_kernel), or, PERM, row * DB + db (the codes kernel,
// whose lane reads the DB codes of one key with one LDS load)
template <int DB, bool PERM> __device__ __forceinline__ int dec_col(int db, int g, int r) { return PERM ? (4 * g + r) * DB + db : 16 * db + 4 * g + r; }

// the waves' partials into wave 0 through LDS, in wave order, then out (one chunk) or the workspace (more); all waves of the workgroup
// call.  c: the lane's column
template <int DT, int D, bool PERM>
__device__ __forceinline__ void dec_finish(char* smem, float m, float l, f32x4_t (&acc)[D / 16], void* out, float* ws, int64_t H, int64_t T, int nsplit,
                                           const DecCol& c) {
    constexpr int DB = D / 16, PART = 4 * DB + 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    // slot e of lane i at float e * 64 + i of the wave's part
    __syncthreads();
    float* part = (float*)smem;
    if (wave > 0) {
        float* mine = part + (wave - 1) * 64 * PART + lane;
        mine[0] = m;
        mine[64] = l;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int r = 0; r < 4; ++r) mine[(2 + 4 * db + r) * 64] = acc[db][r];
        }
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w = 1; w < DEC_WAVES; ++w) {
        const float* theirs = part + (w - 1) * 64 * PART + lane;
        f32x4_t acc1[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc1[db][r] = theirs[(2 + 4 * db + r) * 64];
        }
        dec_merge(m, l, acc, theirs[0], theirs[64], acc1);
    }
    l = dec_sum_groups(l);
    if (!c.live) return;
    if (nsplit == 1) {
        const int64_t o = ((c.b * T + c.t) * H + c.h) * D;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Ty<DT>::store1(out, o + dec_col<DB, PERM>(db, g, r), acc[db][r] / l);
        }
    } else {
        float* w = ws + c.wrow * (D + 2);
        if (g == 0) {
            w[0] = m;
            w[1] = l;
        }
#pragma unroll
        for (int db = 0; db < DB; ++db) {
#pragma unroll
            for (int r = 0; r < 4; ++r) w[2 + dec_col<DB, PERM>(db, g, r)] = acc[db][r];
        }
    }
}

// the whole workgroup's work under either column map; dec_kernel and the grouped kernel (fq_attn_gqa.h) are this body
template <int DT, int MDT, int D, bool VEC, bool GQA>
__device__ __forceinline__ void dec_body(const DecArgs& a) {
    static_assert(D == 64 || D == 128, "head sizes served");
    constexpr int KS = D / 32;                  // k-steps of a score tile
    constexpr int DB = D / 16;                  // 16-column blocks of the output
    constexpr int RS = dec_row_bytes<D>();
    constexpr int STAGE = dec_stage_bytes<D>();
    constexpr int LPR = D / 8;                  // lanes of a V row (16 bytes each)
    constexpr int RPI = 64 / LPR;               // V rows of one load instruction
    constexpr int NVI = DEC_TILE / RPI;         // V load instructions of a tile
    constexpr int PART = 4 * DB + 2;            // floats of a lane's partial
    static_assert((DEC_WAVES - 1) * 64 * PART * 4 <= DEC_WAVES * STAGE, "the merge fits the staging area");
    __shared__ __attribute__((aligned(16))) char smem[DEC_WAVES * STAGE];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const DecCol col = dec_column<GQA>(a, j);       // the lane's query row (dead columns: zero q, never stored)
    const int64_t b = col.b;
    const int64_t S = a.S, last = S - 1;
    const int64_t t0 = (int64_t)blockIdx.y * a.per;
    const int64_t nt = (S + DEC_TILE - 1) / DEC_TILE;
    const int64_t t1 = t0 + a.per < nt ? t0 + a.per : nt;

    const uint16_t* qp = (const uint16_t*)a.q + b * a.qs[0] + col.h * a.qs[1] + col.t * a.qs[2] + 8 * g;
    const uint16_t* kp = (const uint16_t*)a.k + b * a.ks[0] + col.kvh * a.ks[1] + 8 * g;
    const uint16_t* vp = (const uint16_t*)a.v + b * a.vs[0] + col.kvh * a.vs[1] + 8 * (lane % LPR);
    const int64_t mb = MDT == ATTN_NOMASK ? 0 : b * a.mbs + col.t * a.mrs;
    const int vrow = lane / LPR;
    char* stage = smem + wave * STAGE;

    u32x4_t qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const u32x4_t x = dec_ld16<VEC>(qp + 32 * ks);
        qf[ks] = col.live ? x : (u32x4_t){0u, 0u, 0u, 0u};
    }

    auto load_k = [&](int64_t tile, u32x4_t(&kr)[2 * KS]) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            int64_t key = tile * DEC_TILE + 16 * hf + j;
            key = key < last ? key : last;
            const uint16_t* p = kp + key * a.ks[2];
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
            // this tile's V and mask, the next tile's K (clamped: a tile past the chunk re-reads in-range rows and is dropped)
            u32x4_t vr[NVI];
#pragma unroll
            for (int it = 0; it < NVI; ++it) {
                int64_t key = tile * DEC_TILE + it * RPI + vrow;
                key = key < last ? key : last;
                vr[it] = dec_ld16<VEC>(vp + key * a.vs[2]);
            }
            float mk[8];
            dec_load_mask<MDT>(a.mask, mb, tile, g, last, mk);
            u32x4_t kn[2 * KS];
            load_k(tile + DEC_WAVES, kn);

            f32x4_t sc[2];
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
                sc[hf] = (f32x4_t){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) sc[hf] = dec_mfma<DT>(kr[hf * KS + ks], qf[ks], sc[hf]);
            }
            const u32x4_t pf = dec_softmax_step<DT, MDT>(sc, mk, tile, g, S, a.inv, m, l, acc);

            // V through the wave's stage
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

template <int DT, int MDT, int D, bool VEC> __global__ __launch_bounds__(DEC_WAVES * 64) void dec_kernel(DecArgs a) { dec_body<DT, MDT, D, VEC, false>(a); }

// the chunks of one (batch, head, query row) into out, in chunk order: grid (B * H, T), D threads, thread d owns out[.., d].  The chunks'
// (m, l) come in with one load per thread through LDS and the accumulator loads run eight at a time: read one after the other, 2 x 16
// dependent loads of another kernel's fresh output made this kernel as long as the stream it follows
// w: the row's partial of chunk 0, chunk s `step` floats further; o: the row's element of out
template <int DT> __device__ __forceinline__ void dec_combine(const float* w, int64_t step, void* out, int64_t o, int nsplit) {
    static_assert(DEC_MAX_SPLIT <= 64, "a thread per chunk in the smallest block (D = 64)");
    __shared__ float cm[DEC_MAX_SPLIT], cl[DEC_MAX_SPLIT];
    const int d = threadIdx.x;                              // the block is D threads, nsplit <= DEC_MAX_SPLIT <= D
    if (d < nsplit) {
        cm[d] = w[d * step];
        cl[d] = w[d * step + 1];
    }
    __syncthreads();
    float mx = LOSS_NEG_INF;
    for (int s = 0; s < nsplit; ++s) mx = __builtin_fmaxf(mx, cm[s]);
    const float ref = loss_ref(mx);
    float l = 0.0f, acc = 0.0f;
#pragma unroll 8
    for (int s = 0; s < nsplit; ++s) {
        const float f = attn_exp(cm[s] - ref);
        l += cl[s] * f;
        acc += w[s * step + 2 + d] * f;
    }
    Ty<DT>::store1(out, o + d, acc / l);
}
template <int DT> __global__ __launch_bounds__(128) void dec_combine_kernel(const float* ws, void* out, int64_t H, int64_t T, int D, int nsplit) {
    const int64_t bh = blockIdx.x, b = bh / H, h = bh % H, t = blockIdx.y;
    const int64_t row = D + 2, step = T * row;
    dec_combine<DT>(ws + (bh * nsplit * T + t) * row, step, out, ((b * T + t) * H + h) * D, nsplit);
}

}  // namespace fq
