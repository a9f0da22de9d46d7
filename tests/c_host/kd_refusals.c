/* kd_refusals.c -- a plain C host of include/llmqat_fakequant_loss.h that needs no GPU: every call below is refused before any HIP call,
 * so the host side of fql_kd_kl_fwd / fql_kd_kl_bwd can run under the host sanitizers.  Build the library's host code and this file with
 * -fsanitize=address,undefined and run it:
 *
 *   for f in llm-qat_amd/csrc/fq_*.hip; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC \
 *       -Xarch_host -fsanitize=address,undefined -c $f -o san/$(basename $f).o; done
 *   hipcc --offload-arch=gfx950 -shared -fPIC -fsanitize=address,undefined san/*.o -o san/libllmqat_fakequant.so
 *   clang -std=c11 -g -fsanitize=address,undefined -I include tests/c_host/kd_refusals.c -L san -lllmqat_fakequant \
 *       -Wl,-rpath,$PWD/san -o san/kd_refusals && san/kd_refusals
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "llmqat_fakequant_loss.h"

#define EXPECT(call, code, text)                                                                                         \
    do {                                                                                                                 \
        const int rc_ = (call);                                                                                          \
        if (rc_ != (code) || !strstr(fq_last_error(), (text))) {                                                         \
            fprintf(stderr, "%s:%d %s -> %d \"%s\", expected %d \"%s\"\n", __FILE__, __LINE__, #call, rc_, fq_last_error(), (code), (text)); \
            return 1;                                                                                                    \
        }                                                                                                                \
    } while (0)

int main(void) {
    void* const S = (void*)(uintptr_t)0x1000; /* never dereferenced; no pointer needs an alignment */
    void* const T = (void*)(uintptr_t)0x2002;
    float* const ST = (float*)(uintptr_t)0x3004;
    float* const RL = (float*)(uintptr_t)0x4004;
    float* const LO = (float*)(uintptr_t)0x5004;
    float* const G = (float*)(uintptr_t)0x6004;
    void* const GS = (void*)(uintptr_t)0x7002;
    const int64_t big = (int64_t)1 << 62;
    /* the header's order: each call is valid up to the check it names and wrong in everything behind it */
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, -1, -1, 0, 9, NULL), FQ_ERR_DTYPE, "unknown dtype");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, -1, -1, 0, -1, NULL), FQ_ERR_DTYPE, "unknown dtype");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, -1, -1, 0, FQ_DTYPE_F64, NULL), FQ_ERR_DTYPE, "float64");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, -3, 8, 0, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "negative shape");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, 3, -8, 0, FQ_DTYPE_F16, NULL), FQ_ERR_SHAPE, "negative shape");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, 0, 8, 0, FQ_DTYPE_F32, NULL), FQ_ERR_SHAPE, "empty shape");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, 3, 0, 0, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "empty shape");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, big, (int64_t)1 << 40, 0, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "overflows");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, 3, 8, 0, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "batch=0");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, 3, 8, -2, FQ_DTYPE_F32, NULL), FQ_ERR_ARG, "batch=-2");
    EXPECT(fql_kd_kl_fwd(NULL, T, ST, RL, LO, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_fwd(S, NULL, ST, RL, LO, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_fwd(S, T, ST, NULL, LO, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_fwd(S, T, ST, RL, NULL, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_fwd(NULL, NULL, NULL, NULL, NULL, (int64_t)1 << 40, 32000, 1, FQ_DTYPE_F16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_fwd(S, T, NULL, RL, LO, (int64_t)1 << 33, 2048, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");
    EXPECT(fql_kd_kl_fwd(S, T, ST, RL, LO, (int64_t)1 << 34, 8, 1, FQ_DTYPE_F32, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");

    EXPECT(fql_kd_kl_bwd(NULL, NULL, NULL, NULL, NULL, -1, -1, 0, 9, NULL), FQ_ERR_DTYPE, "unknown dtype");
    EXPECT(fql_kd_kl_bwd(NULL, NULL, NULL, NULL, NULL, -1, -1, 0, FQ_DTYPE_F64, NULL), FQ_ERR_DTYPE, "float64");
    EXPECT(fql_kd_kl_bwd(NULL, NULL, NULL, NULL, NULL, -3, 8, 0, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "negative shape");
    EXPECT(fql_kd_kl_bwd(NULL, NULL, NULL, NULL, NULL, 0, 8, 0, FQ_DTYPE_F32, NULL), FQ_ERR_SHAPE, "empty shape");
    EXPECT(fql_kd_kl_bwd(NULL, NULL, NULL, NULL, NULL, big, (int64_t)1 << 40, 0, FQ_DTYPE_BF16, NULL), FQ_ERR_SHAPE, "overflows");
    EXPECT(fql_kd_kl_bwd(NULL, NULL, NULL, NULL, NULL, 3, 8, 0, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "batch=0");
    EXPECT(fql_kd_kl_bwd(NULL, T, ST, G, GS, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_bwd(S, NULL, ST, G, GS, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_bwd(S, T, NULL, G, GS, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_bwd(S, T, ST, NULL, GS, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_bwd(S, T, ST, G, NULL, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_NULL, "NULL");
    EXPECT(fql_kd_kl_bwd(S, T, ST, G, S, 3, 8, 1, FQ_DTYPE_BF16, NULL), FQ_ERR_ARG, "in-place");
    EXPECT(fql_kd_kl_bwd(S, T, ST, G, T, (int64_t)1 << 34, 8, 1, FQ_DTYPE_F32, NULL), FQ_ERR_ARG, "in-place");
    EXPECT(fql_kd_kl_bwd(S, T, ST, G, GS, (int64_t)1 << 34, 8, 1, FQ_DTYPE_F32, NULL), FQ_ERR_UNSUPPORTED, "exceed one launch's grid");
    printf("kd_refusals ok\n");
    return 0;
}
