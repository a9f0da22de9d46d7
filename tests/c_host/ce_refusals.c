/* ce_refusals.c -- a plain C host of include/llmqat_fakequant_ce.h that needs no GPU: every call below is refused before any HIP call,
 * so the host side of fqc_ce_fwd / fqc_ce_bwd can run under the host sanitizers.  Build the library's host code and this file with
 * -fsanitize=address,undefined and run it (the recipe of kd_refusals.c, with this file in its last line):
 *
 *   for f in llm-qat_amd/csrc/fq_*.hip; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC \
 *       -Xarch_host -fsanitize=address,undefined -c $f -o san/$(basename $f).o; done
 *   hipcc --offload-arch=gfx950 -shared -fPIC -fsanitize=address,undefined san/*.o -o san/libllmqat_fakequant.so
 *   clang -std=c11 -g -fsanitize=address,undefined -I include tests/c_host/ce_refusals.c -L san -lllmqat_fakequant \
 *       -Wl,-rpath,$PWD/san -o san/ce_refusals && san/ce_refusals
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "llmqat_fakequant_ce.h"

#define EXPECT(call, code, text)                                                                                         \
    do {                                                                                                                 \
        const int rc_ = (call);                                                                                          \
        if (rc_ != (code) || !strstr(fq_last_error(), (text))) {                                                         \
            fprintf(stderr, "%s:%d %s -> %d \"%s\", expected %d \"%s\"\n", __FILE__, __LINE__, #call, rc_, fq_last_error(), (code), (text)); \
            return 1;                                                                                                    \
        }                                                                                                                \
    } while (0)

#define MEAN FQC_REDUCTION_MEAN
#define SUM FQC_REDUCTION_SUM

int main(void) {
    void* const X = (void*)(uintptr_t)0x1000; /* never dereferenced; no pointer needs an alignment here */
    int64_t* const LAB = (int64_t*)(uintptr_t)0x2008;
    float* const LSE = (float*)(uintptr_t)0x3004;
    float* const RL = (float*)(uintptr_t)0x4004;
    float* const LO = (float*)(uintptr_t)0x5004;
    void* const NV = (void*)(uintptr_t)0x6008;
    float* const G = (float*)(uintptr_t)0x7004;
    void* const GX = (void*)(uintptr_t)0x8002;
    const int64_t big = (int64_t)1 << 62;
    /* the header's order: each call is valid up to the check it names and wrong in everything behind it */
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, -1, -1, 0, 7, -100, 9, 9, NULL), FQ_ERR_DTYPE, "unknown dtype");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, -1, -1, 0, 7, -100, 9, -1, NULL), FQ_ERR_DTYPE, "unknown dtype");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, -1, -1, 0, 7, -100, 9, FQ_DTYPE_F64, NULL), FQ_ERR_DTYPE, "float64");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, -3, 8, 0, 7, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "negative shape");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, 3, -8, 0, 7, -100, 9, FQ_DTYPE_F16, NULL), FQ_ERR_SHAPE, "negative shape");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, 0, 8, 0, 7, -100, 9, FQ_DTYPE_F32, NULL), FQ_ERR_SHAPE, "empty shape");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, 3, 0, 0, 7, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "empty shape");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, big, (int64_t)1 << 40, 0, 7, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "overflows");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, 7, 8, 3, 1, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "not whole sequences");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, 6, 8, 3, 2, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "shift=2");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, 6, 8, 0, 1, -100, 9, FQ_DTYPE_F32, NULL), FQ_ERR_ARG, "unknown reduction");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, 6, 8, 0, 1, -100, SUM, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "seq_len=0");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, 6, 8, -3, 0, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "seq_len=-3");
    EXPECT(fqc_ce_fwd(NULL, LAB, LSE, RL, LO, NV, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_fwd(X, NULL, LSE, RL, LO, NV, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_fwd(X, LAB, LSE, NULL, LO, NV, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_fwd(X, LAB, LSE, RL, NULL, NV, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_fwd(X, LAB, LSE, RL, LO, NULL, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_fwd(NULL, NULL, NULL, NULL, NULL, NULL, (int64_t)1 << 40, 32000, (int64_t)1 << 20, 1, -100, SUM, FQ_DTYPE_F16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_fwd(X, LAB, NULL, RL, LO, NV, (int64_t)1 << 33, 2048, 2048, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");
    EXPECT(fqc_ce_fwd(X, LAB, LSE, RL, LO, NV, (int64_t)1 << 34, 8, 1, 0, -100, SUM, FQ_DTYPE_F32, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");

    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, -1, -1, 0, 7, -100, 9, 9, NULL), FQ_ERR_DTYPE, "unknown dtype");
    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, -1, -1, 0, 7, -100, 9, FQ_DTYPE_F64, NULL), FQ_ERR_DTYPE, "float64");
    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, -3, 8, 0, 7, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "negative shape");
    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, 0, 8, 0, 7, -100, 9, FQ_DTYPE_F32, NULL), FQ_ERR_SHAPE, "empty shape");
    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, big, (int64_t)1 << 40, 0, 7, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "overflows");
    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, 7, 8, 3, 1, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "not whole sequences");
    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, 6, 8, 3, 2, -100, 9, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "shift=2");
    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, 6, 8, 0, 1, -100, 9, FQ_DTYPE_F32, NULL), FQ_ERR_ARG, "unknown reduction");
    EXPECT(fqc_ce_bwd(NULL, NULL, NULL, NULL, NULL, NULL, 6, 8, 0, 1, -100, SUM, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "seq_len=0");
    EXPECT(fqc_ce_bwd(NULL, LAB, LSE, NV, G, GX, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_bwd(X, NULL, LSE, NV, G, GX, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_bwd(X, LAB, NULL, NV, G, GX, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_bwd(X, LAB, LSE, NULL, G, GX, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_bwd(X, LAB, LSE, NV, NULL, GX, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_bwd(X, LAB, LSE, NV, G, NULL, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fqc_ce_bwd(X, LAB, LSE, NV, G, X, 6, 8, 3, 1, -100, MEAN, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "in-place");
    EXPECT(fqc_ce_bwd(X, LAB, LSE, NV, G, X, (int64_t)1 << 34, 8, 1, 0, -100, SUM, FQ_DTYPE_F32, NULL), FQ_ERR_ARG, "in-place");
    EXPECT(fqc_ce_bwd(X, LAB, LSE, NV, G, GX, (int64_t)1 << 34, 8, 1, 0, -100, SUM, FQ_DTYPE_F32, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");
    printf("ce_refusals ok\n");
    return 0;
}
