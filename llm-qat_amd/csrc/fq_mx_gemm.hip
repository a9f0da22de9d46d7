// fq_mx_gemm.hip -- the MX block-scaled GEMM kernels (fq_mx_gemm.h), all 9 operand format pairs: a translation unit of its own, so the
// other units compile exactly as before.
#include "fq_mx_gemm.h"
