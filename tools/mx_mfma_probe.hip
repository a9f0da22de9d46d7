// mx_mfma_probe.hip -- the operand layout of v_mfma_scale_f32_16x16x128_f8f6f4 on gfx950, established with exact integer data.
//
//   hipcc --offload-arch=gfx950 -O2 -o tools/mx_mfma_probe tools/mx_mfma_probe.hip && tools/mx_mfma_probe > profiles/mx_mfma_layout.txt
//
// One wave per case.  Element map: one operand is one-hot (a single 1.0 at byte / nibble j of lane L, everything else 0), the other is
// 1.0 or 2.0 everywhere, 2.0 where bit p of its hypothesised k (passes 0..6) or of its hypothesised row / column (passes 7..10) is set.
// The position of the nonzero row (column) of D gives the one-hot element's row (column); the values decode its k as seen by the other
// operand, and passes 7..10 check the other
// operand's row / column against D's.  The map the probe checks (it prints every case that differs), with g = l >> 4:
//   fp4 operand  lane l, nibble j (low nibble of byte j / 2 first) is row (column) l & 15, k = 32 * g + j;
//   fp8 operand  lane l, byte j is row (column) l & 15, k = 16 * g + j for j < 16 and 64 + 16 * g + (j - 16) for j >= 16:
//                the operand's low 4 dwords are the k < 64 half of the step, its high 4 dwords the k >= 64 half;
//   scale        lane l's byte (the one op_sel picks) scales row (column) l & 15 over k = 32 * g .. 32 * g + 31, whatever the format.
// Scale map: all elements 1.0, lane l's scale byte 127 + l in the selected byte of the scale register, decoys in the other three; the
// other operand's ones are confined to one k block, so D / 32 is a power of two that names the lane whose scale reached (row, block).
// Then a 0xFF scale byte, scale bytes 0 and 254, and an E4M3 NaN element.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                \
            exit(2);                                                               \
        }                                                                          \
    } while (0)

// format codes of cbsz (A) / blgp (B): 0 e4m3, 1 e5m2, 4 e2m1
template <int FA, int FB, int OPA, int OPB> __device__ f32x4 mma(i32x8 a, i32x8 b, int sa, int sb) {
    f32x4 c = {0.f, 0.f, 0.f, 0.f};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, FA, FB, OPA, sa, OPB, sb);
}

__device__ uint32_t one_code(int f) { return f == 4 ? 0x2u : f == 0 ? 0x38u : 0x3Cu; }   // 1.0
__device__ uint32_t two_code(int f) { return f == 4 ? 0x4u : f == 0 ? 0x40u : 0x40u; }   // 2.0

// k of element j of lane l's fragment (the map under test)
__host__ __device__ int k_of(int f, int l, int j) {
    const int g = l >> 4;
    return f == 4 ? 32 * g + j : j < 16 ? 16 * g + j : 64 + 16 * g + (j - 16);
}

// element j of a fragment <- code (fp8: byte j; fp4: nibble j, low nibble first)
__device__ void put(i32x8& v, int f, int j, uint32_t code) {
    uint32_t w[8];
    for (int i = 0; i < 8; ++i) w[i] = (uint32_t)v[i];
    if (f == 4) w[j >> 3] |= code << (4 * (j & 7));
    else w[j >> 2] |= code << (8 * (j & 3));
    for (int i = 0; i < 8; ++i) v[i] = (int)w[i];
}

// out[case][pass][lane][4]; case = L * 32 + j.  HOT_A: the one-hot operand is A (else B); F1 its format, F2 the other operand's.
template <int F1, int F2, bool HOT_A> __global__ void elem_probe(float* out) {
    const int cs = blockIdx.x, L = cs >> 5, j = cs & 31, l = threadIdx.x;
    i32x8 hot = {0, 0, 0, 0, 0, 0, 0, 0};
    if (l == L) put(hot, F1, j, one_code(F1));
    for (int p = 0; p < 11; ++p) {
        i32x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int e = 0; e < 32; ++e) {
            const int k = k_of(F2, l, e), idx = l & 15;
            const int bit = p < 7 ? (k >> p) & 1 : (idx >> (p - 7)) & 1;
            put(o, F2, e, bit ? two_code(F2) : one_code(F2));
        }
        f32x4 d;
        if (HOT_A) d = mma<F1, F2, 0, 0>(hot, o, 127, 127);
        else d = mma<F2, F1, 0, 0>(o, hot, 127, 127);
        float* q = out + (((size_t)cs * 11 + p) * 64 + l) * 4;
        q[0] = d[0], q[1] = d[1], q[2] = d[2], q[3] = d[3];
    }
}

// mode 0..3: A scale of lane l = 127 + l in byte `mode` (op_sel mode), B's ones confined to k block blockIdx.x; mode 4..7: the same for B.
// out[blk][mode][lane][4]
__global__ void scale_probe(float* out) {
    const int kb = blockIdx.x, l = threadIdx.x;
    i32x8 ones = {0, 0, 0, 0, 0, 0, 0, 0}, conf = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = 0; e < 32; ++e) {
        put(ones, 0, e, 0x38u);
        if (k_of(0, l, e) / 32 == kb) put(conf, 0, e, 0x38u);
    }
    for (int mode = 0; mode < 8; ++mode) {
        const int byte = mode & 3;
        const int s = ((127 + l) & 0xFF) << (8 * byte) | (~(0xFF << (8 * byte)) & 0x11223344);   // decoys in the other bytes
        f32x4 d;
        switch (mode) {
            case 0: d = mma<0, 0, 0, 0>(ones, conf, s, 127); break;
            case 1: d = mma<0, 0, 1, 0>(ones, conf, s, 127); break;
            case 2: d = mma<0, 0, 2, 0>(ones, conf, s, 127); break;
            case 3: d = mma<0, 0, 3, 0>(ones, conf, s, 127); break;
            case 4: d = mma<0, 0, 0, 0>(conf, ones, 127, s); break;
            case 5: d = mma<0, 0, 0, 1>(conf, ones, 127, s); break;
            case 6: d = mma<0, 0, 0, 2>(conf, ones, 127, s); break;
            default: d = mma<0, 0, 0, 3>(conf, ones, 127, s); break;
        }
        float* q = out + (((size_t)kb * 8 + mode) * 64 + l) * 4;
        q[0] = d[0], q[1] = d[1], q[2] = d[2], q[3] = d[3];
    }
}

// special scale bytes.  case 0: A scale 0xFF in lane 5 only, all elements 1.0; 1: the same with A's elements all 0; 2: B scale 0xFF in
// lane 21; 3: A scale 0 (2^-127) x B scale 254 (2^127), all elements 1.0 (expected 128); 4: A scale 0, B scale 127 (expected 128 * 2^-127,
// a subnormal fp32); 5: A e4m3 NaN code 0x7F in lane 3 byte 0, scales 1.  out[case][lane][4]
__global__ void special_probe(float* out) {
    const int cs = blockIdx.x, l = threadIdx.x;
    i32x8 ones = {0, 0, 0, 0, 0, 0, 0, 0}, zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int e = 0; e < 32; ++e) put(ones, 0, e, 0x38u);
    f32x4 d;
    if (cs == 0) d = mma<0, 0, 0, 0>(ones, ones, l == 5 ? 0xFF : 127, 127);
    else if (cs == 1) d = mma<0, 0, 0, 0>(zero, ones, l == 5 ? 0xFF : 127, 127);
    else if (cs == 2) d = mma<0, 0, 0, 0>(ones, ones, 127, l == 21 ? 0xFF : 127);
    else if (cs == 3) d = mma<0, 0, 0, 0>(ones, ones, 0, 254);
    else if (cs == 4) d = mma<0, 0, 0, 0>(ones, ones, 0, 127);
    else {
        i32x8 a = ones;
        if (l == 3) a[0] = (a[0] & ~0xFF) | 0x7F;
        d = mma<0, 0, 0, 0>(a, ones, 127, 127);
    }
    float* q = out + ((size_t)cs * 64 + l) * 4;
    q[0] = d[0], q[1] = d[1], q[2] = d[2], q[3] = d[3];
}

// D as a 16 x 16 matrix from the per-lane registers: row = 4 * (lane >> 4) + i, col = lane & 15
static void to_matrix(const float* lanes, float D[16][16]) {
    for (int l = 0; l < 64; ++l)
        for (int i = 0; i < 4; ++i) D[4 * (l >> 4) + i][l & 15] = lanes[l * 4 + i];
}

template <int F1, int F2, bool HOT_A> static int run_elem(const char* name) {
    const size_t n = (size_t)2048 * 11 * 256;
    float* d;
    CK(hipMalloc(&d, n * sizeof(float)));
    elem_probe<F1, F2, HOT_A><<<2048, 64>>>(d);
    CK(hipDeviceSynchronize());
    std::vector<float> h(n);
    CK(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
    CK(hipFree(d));
    int bad = 0;
    printf("== %s\n", name);
    for (int cs = 0; cs < 2048; ++cs) {
        const int L = cs >> 5, j = cs & 31;
        int idx = -1, k = 0, oidx_ok = 1, shape_ok = 1;
        float D[16][16];
        for (int p = 0; p < 11; ++p) {
            to_matrix(&h[((size_t)cs * 11 + p) * 256], D);
            // the one-hot element's row (HOT_A) / column: the only line of D that is nonzero
            int line = -1, nlines = 0;
            for (int a = 0; a < 16; ++a) {
                int nz = 0;
                for (int b = 0; b < 16; ++b) nz += (HOT_A ? D[a][b] : D[b][a]) != 0.f;
                if (nz) line = a, ++nlines, shape_ok &= nz == 16;
            }
            shape_ok &= nlines == 1;
            if (nlines != 1) break;
            if (p == 0) idx = line;
            shape_ok &= line == idx;
            for (int b = 0; b < 16; ++b) {
                const float v = HOT_A ? D[line][b] : D[b][line];
                shape_ok &= v == 1.f || v == 2.f;
                if (p < 7) {
                    if (b == 0) k |= (v == 2.f) << p;
                    shape_ok &= (v == 2.f) == ((k >> p) & 1);
                } else {
                    oidx_ok &= (v == 2.f) == ((b >> (p - 7)) & 1);
                }
            }
        }
        const int ok = shape_ok && oidx_ok && idx == (L & 15) && k == k_of(F1, L, j);
        bad += !ok;
        if (!ok || (j == 0 && (L & 15) == 0) || (L == 37 && j < 4))
            printf("lane %2d elem %2d -> %s %2d k %3d  shape_ok %d other_index_ok %d %s\n", L, j, HOT_A ? "row" : "col", idx, k, shape_ok, oidx_ok,
                   ok ? "" : "MISMATCH");
    }
    printf("%s: %d of 2048 (lane, element) cases differ from the map in this file's header\n", name, bad);
    return bad;
}

int main() {
    int dev = 0;
    hipDeviceProp_t pr;
    CK(hipGetDeviceProperties(&pr, dev));
    printf("device %s (%s)\n", pr.name, pr.gcnArchName);
    printf("instruction: v_mfma_scale_f32_16x16x128_f8f6f4; D: row = 4 * (lane >> 4) + reg, col = lane & 15 (assumed, shape-determined)\n");
    int bad = 0;
    bad += run_elem<0, 0, true>("A e4m3 (byte j), B e4m3");
    bad += run_elem<0, 0, false>("B e4m3 (byte j), A e4m3");
    bad += run_elem<4, 0, true>("A e2m1 (nibble j, low nibble first), B e4m3");
    bad += run_elem<4, 0, false>("B e2m1 (nibble j, low nibble first), A e4m3");
    bad += run_elem<4, 4, true>("A e2m1, B e2m1");
    bad += run_elem<1, 4, true>("A e5m2 (byte j), B e2m1");
    bad += run_elem<1, 0, false>("B e5m2 (byte j), A e4m3");

    {
        const size_t n = 4 * 8 * 256;
        float* d;
        CK(hipMalloc(&d, n * sizeof(float)));
        scale_probe<<<4, 64>>>(d);
        CK(hipDeviceSynchronize());
        std::vector<float> h(n);
        CK(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
        CK(hipFree(d));
        printf("== scale operand: lane l carries 127 + l in byte op_sel; entry = the lane whose scale reached (index, k block)\n");
        for (int mode = 0; mode < 8; ++mode) {
            int sbad = 0;
            printf("%c scale, op_sel %d:\n", mode < 4 ? 'A' : 'B', mode & 3);
            for (int kb = 0; kb < 4; ++kb) {
                float D[16][16];
                to_matrix(&h[((size_t)kb * 8 + mode) * 256], D);
                printf("  k block %d:", kb);
                for (int a = 0; a < 16; ++a) {
                    const float v = mode < 4 ? D[a][0] : D[0][a];
                    int uniform = 1;
                    for (int b = 0; b < 16; ++b) uniform &= (mode < 4 ? D[a][b] : D[b][a]) == v;
                    const float lg = log2f(v / 32.f);
                    const int lane = (int)lg;
                    const int ok = uniform && lg == (float)lane && lane == 16 * kb + a;
                    sbad += !ok;
                    printf(" %d%s", lane, ok ? "" : "!");
                }
                printf("\n");
            }
            printf("  %d of 64 differ from  lane = 16 * block + index\n", sbad);
            bad += sbad;
        }
    }
    {
        const size_t n = 6 * 256;
        float* d;
        CK(hipMalloc(&d, n * sizeof(float)));
        special_probe<<<6, 64>>>(d);
        CK(hipDeviceSynchronize());
        std::vector<float> h(n);
        CK(hipMemcpy(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost));
        CK(hipFree(d));
        const char* names[6] = {"A scale 0xFF in lane 5, elements 1.0", "A scale 0xFF in lane 5, A elements 0", "B scale 0xFF in lane 21, elements 1.0",
                                "A scale 0 x B scale 254, elements 1.0 (exact value 128)", "A scale 0 x B scale 127 (exact value 128 * 2^-127)",
                                "A e4m3 NaN code in lane 3 byte 0"};
        printf("== special values\n");
        for (int cs = 0; cs < 6; ++cs) {
            float D[16][16];
            to_matrix(&h[(size_t)cs * 256], D);
            int nan = 0;
            for (int a = 0; a < 16; ++a)
                for (int b = 0; b < 16; ++b) nan += std::isnan(D[a][b]);
            printf("%s: %d NaN of 256;", names[cs], nan);
            printf(" D[5][0] %g D[5][7] %g D[3][2] %g D[0][5] %g D[0][0] %g D[9][9] %g (bits %08x)\n", D[5][0], D[5][7], D[3][2], D[0][5], D[0][0], D[9][9],
                   [&] { uint32_t u; memcpy(&u, &D[9][9], 4); return u; }());
            if (nan && nan < 256) {
                printf("  NaN rows:");
                for (int a = 0; a < 16; ++a) {
                    int c = 0;
                    for (int b = 0; b < 16; ++b) c += std::isnan(D[a][b]);
                    if (c) printf(" %d(%d)", a, c);
                }
                printf("  NaN cols:");
                for (int b = 0; b < 16; ++b) {
                    int c = 0;
                    for (int a = 0; a < 16; ++a) c += std::isnan(D[a][b]);
                    if (c) printf(" %d(%d)", b, c);
                }
                printf("\n");
            }
        }
    }
    printf("total mismatches against the map: %d\n", bad);
    return 0;
}
