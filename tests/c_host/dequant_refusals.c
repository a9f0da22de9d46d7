/* dequant_refusals.c -- a plain C host of include/llmqat_fakequant_infer.h that needs no GPU: every call below is refused (or is an
 * empty shape) before any HIP call, so the host side of fqi_mx_dequant can run under the host sanitizers.  Build the library's host code
 * and this file with -fsanitize=address,undefined and run it:
 *
 *   for f in llm-qat_amd/csrc/fq_*.hip; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC \
 *       -Xarch_host -fsanitize=address,undefined -c $f -o san/$(basename $f).o; done
 *   hipcc --offload-arch=gfx950 -shared -fPIC -fsanitize=address,undefined san/*.o -o san/libllmqat_fakequant.so
 *   clang -std=c11 -g -fsanitize=address,undefined -I include tests/c_host/dequant_refusals.c -L san -lllmqat_fakequant \
 *       -Wl,-rpath,$PWD/san -o san/dequant_refusals && san/dequant_refusals
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "llmqat_fakequant_infer.h"

#define EXPECT(call, code, text)                                                                                         \
    do {                                                                                                                 \
        const int rc_ = (call);                                                                                          \
        if (rc_ != (code) || !strstr(fq_last_error(), (text))) {                                                         \
            fprintf(stderr, "%s:%d %s -> %d \"%s\", expected %d \"%s\"\n", __FILE__, __LINE__, #call, rc_, fq_last_error(), (code), (text)); \
            return 1;                                                                                                    \
        }                                                                                                                \
    } while (0)

int main(void) {
    void* const A = (void*)(uintptr_t)0x1000; /* 16-byte aligned, never dereferenced */
    void* const B = (void*)(uintptr_t)0x2000;
    void* const S = (void*)(uintptr_t)0x3001; /* the scales need no alignment */
    void* const A2 = (void*)(uintptr_t)0x1002;
    const int64_t big = (int64_t)1 << 62;
    /* the header's order: each call is valid up to the check it names and wrong in everything behind it */
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, -1, -1, 9, 9, NULL), FQ_ERR_DTYPE, "unknown dtype");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, -1, -1, 9, -1, NULL), FQ_ERR_DTYPE, "unknown dtype");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, -1, -1, 9, FQ_DTYPE_F64, NULL), FQ_ERR_DTYPE, "float64");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, -1, -1, 5, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "unknown MX format");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, -1, -1, -1, FQ_DTYPE_F32, NULL), FQ_ERR_ARG, "unknown MX format");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, -1, -1, FQ_MX_FP6_E2M3, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "FP6 formats have no export packing");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, -1, 33, FQ_MX_FP6_E3M2, FQ_DTYPE_F16, NULL), FQ_ERR_ARG, "FP6 formats have no export packing");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, -3, 32, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "negative shape");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, 3, -32, FQ_MX_FP8_E4M3, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "negative shape");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, 3, 33, FQ_MX_FP8_E4M3, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "not a multiple of the 32");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, 0, 16, FQ_MX_FP8_E5M2, FQ_DTYPE_F32, NULL), FQ_ERR_SHAPE, "not a multiple of the 32");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, big, (int64_t)1 << 40, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "overflows");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, 0, 32, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, NULL), FQ_OK, "");
    EXPECT(fqi_mx_dequant(NULL, NULL, NULL, 3, 0, FQ_MX_FP8_E5M2, FQ_DTYPE_F16, NULL), FQ_OK, "");
    EXPECT(fqi_mx_dequant(NULL, S, B, 3, 32, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqi_mx_dequant(A, NULL, B, 3, 32, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqi_mx_dequant(A, S, NULL, 3, 32, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqi_mx_dequant(A2, S, B, 3, 32, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, NULL), FQ_ERR_UNSUPPORTED, "16-byte aligned");
    EXPECT(fqi_mx_dequant(A, S, A2, 3, 32, FQ_MX_FP8_E5M2, FQ_DTYPE_F32, NULL), FQ_ERR_UNSUPPORTED, "16-byte aligned");
    EXPECT(fqi_mx_dequant(A2, S, B, (int64_t)1 << 45, (int64_t)1 << 14, FQ_MX_FP8_E4M3, FQ_DTYPE_F16, NULL), FQ_ERR_UNSUPPORTED, "16-byte aligned");
    EXPECT(fqi_mx_dequant(A, S, B, (int64_t)1 << 45, (int64_t)1 << 14, FQ_MX_FP4_E2M1, FQ_DTYPE_BF16, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");
    printf("dequant_refusals ok\n");
    return 0;
}
