/* sr_refusals.c -- a plain C host of include/llmqat_fakequant_sr.h that needs no GPU: every call below is refused (or is an empty
 * shape, or the host-only noise function) before any HIP call, so the host side of the three fqs_ entry points can run under the host
 * sanitizers.  Build the library's host code and this file with -fsanitize=address,undefined and run it:
 *
 *   for f in llm-qat_amd/csrc/fq_*.hip; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC \
 *       -Xarch_host -fsanitize=address,undefined -c $f -o san/$(basename $f).o; done
 *   hipcc --offload-arch=gfx950 -shared -fPIC -fsanitize=address,undefined san/*.o -o san/libllmqat_fakequant.so
 *   clang -std=c11 -g -fsanitize=address,undefined -I include tests/c_host/sr_refusals.c -L san -lllmqat_fakequant \
 *       -Wl,-rpath,$PWD/san -o san/sr_refusals && san/sr_refusals
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "llmqat_fakequant_sr.h"

#define EXPECT(call, code, text)                                                                                         \
    do {                                                                                                                 \
        const int rc_ = (call);                                                                                          \
        if (rc_ != (code) || !strstr(fq_last_error(), (text))) {                                                         \
            fprintf(stderr, "%s:%d %s -> %d \"%s\", expected %d \"%s\"\n", __FILE__, __LINE__, #call, rc_, fq_last_error(), (code), (text)); \
            return 1;                                                                                                    \
        }                                                                                                                \
    } while (0)

typedef int (*sr_fn)(const void*, void*, int64_t, int64_t, int, int, int, uint64_t, uint64_t, void*);

int main(void) {
    void* const A = (void*)(uintptr_t)0x1000; /* 16-byte aligned, never dereferenced */
    void* const B = (void*)(uintptr_t)0x2000;
    void* const A2 = (void*)(uintptr_t)0x1002;
    const uint64_t all = ~(uint64_t)0;
    const sr_fn fns[2] = {fqs_mx_fwd, fqs_mx_fwd_cols};
    for (int k = 0; k < 2; ++k) {
        const sr_fn f = fns[k];
        const int64_t rows = k ? 32 : 3, cols = k ? 8 : 32; /* a shape each entry point takes */
        EXPECT(f(NULL, NULL, -1, -1, 9, 9, 4, all, all, NULL), FQ_ERR_DTYPE, "unknown dtype");
        EXPECT(f(NULL, NULL, -1, -1, 9, FQ_DTYPE_F64, 4, 0, 0, NULL), FQ_ERR_DTYPE, "float64");
        EXPECT(f(NULL, NULL, -1, -1, 5, FQ_DTYPE_BF16, 4, 1, 2, NULL), FQ_ERR_ARG, "unknown MX format");
        EXPECT(f(NULL, NULL, -1, -1, FQ_MX_FP8_E4M3, FQ_DTYPE_BF16, FQ_MX_FLAG_ROTATE, 1, 2, NULL), FQ_ERR_ARG, "flag bits 0x1");
        EXPECT(f(NULL, NULL, -rows, cols, FQ_MX_FP4_E2M1, FQ_DTYPE_F16, 0, 1, 2, NULL), FQ_ERR_SHAPE, "negative shape");
        EXPECT(f(NULL, NULL, 33, 33, FQ_MX_FP4_E2M1, FQ_DTYPE_F32, FQ_MX_FLAG_CEIL, 1, 2, NULL), FQ_ERR_SHAPE, "not a multiple of the 32");
        EXPECT(f(NULL, NULL, (int64_t)1 << 62, (int64_t)1 << 40, FQ_MX_FP4_E2M1, FQ_DTYPE_F32, 0, 1, 2, NULL), FQ_ERR_SHAPE, "overflows");
        EXPECT(f(NULL, NULL, 0, cols, FQ_MX_FP6_E2M3, FQ_DTYPE_BF16, 0, all, 0, NULL), FQ_OK, "");
        EXPECT(f(NULL, NULL, rows, 0, FQ_MX_FP6_E3M2, FQ_DTYPE_BF16, 0, 0, all, NULL), FQ_OK, "");
        EXPECT(f(NULL, B, rows, cols, FQ_MX_FP8_E5M2, FQ_DTYPE_BF16, 0, 1, 2, NULL), FQ_ERR_NULL, "NULL");
        EXPECT(f(A, NULL, rows, cols, FQ_MX_FP8_E5M2, FQ_DTYPE_BF16, 0, 1, 2, NULL), FQ_ERR_NULL, "NULL");
        EXPECT(f(A2, A2, rows, cols, FQ_MX_FP8_E5M2, FQ_DTYPE_BF16, 0, 1, 2, NULL), FQ_ERR_ARG, "in-place");
        EXPECT(f(A2, B, rows, cols, FQ_MX_FP8_E5M2, FQ_DTYPE_BF16, 0, 1, 2, NULL), FQ_ERR_UNSUPPORTED, "16-byte aligned");
    }
    EXPECT(fqs_mx_fwd(A, B, (int64_t)1 << 45, (int64_t)1 << 14, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, 0, 1, 2, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");
    EXPECT(fqs_mx_fwd_cols(A, B, 32, 7, FQ_MX_FP4_E2M1, FQ_DTYPE_F16, 0, 1, 2, NULL), FQ_ERR_UNSUPPORTED, "whole 16-byte vectors");
    EXPECT(fqs_mx_fwd_cols(A, B, (int64_t)1 << 36, 8, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, 0, 1, 2, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");

    /* the host-only noise: counter 0 of key 0 is the generator's first known answer, low half of each word first */
    uint16_t out[8];
    EXPECT(fqs_mx_noise(0, 0, 0, 8, FQ_DTYPE_BF16, out), FQ_OK, "");
    const uint32_t want[4] = {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u};
    for (int j = 0; j < 8; ++j)
        if (out[j] != (uint16_t)(want[j >> 1] >> (16 * (j & 1)))) {
            fprintf(stderr, "fqs_mx_noise: element %d is %04x\n", j, out[j]);
            return 2;
        }
    uint16_t* big = malloc(1000 * sizeof *big);  /* a heap buffer, so that a write past n would be seen */
    if (!big) return 3;
    EXPECT(fqs_mx_noise(all, all, ((int64_t)1 << 40) + 3, 1000, FQ_DTYPE_F32, big), FQ_OK, "");
    EXPECT(fqs_mx_noise(all, all, INT64_MAX - 1000, 1000, FQ_DTYPE_F16, big), FQ_OK, "");
    EXPECT(fqs_mx_noise(1, 2, -1, 4, FQ_DTYPE_BF16, big), FQ_ERR_SHAPE, "negative range");
    EXPECT(fqs_mx_noise(1, 2, INT64_MAX, 4, FQ_DTYPE_BF16, big), FQ_ERR_SHAPE, "overflows");
    EXPECT(fqs_mx_noise(1, 2, 0, ((int64_t)1 << 24) + 1, FQ_DTYPE_BF16, big), FQ_ERR_SHAPE, "at most 2^24");
    EXPECT(fqs_mx_noise(1, 2, 0, 4, FQ_DTYPE_F64, big), FQ_ERR_DTYPE, "float64");
    EXPECT(fqs_mx_noise(1, 2, 0, 4, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    free(big);
    printf("sr_refusals ok\n");
    return 0;
}
