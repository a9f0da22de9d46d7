// fq_mx_dequant.hip -- instantiations of the MX dequantize kernel (fq_mx_dequant.h) for the three output types: a translation unit of its
// own, so the other units compile exactly as before.
#include "fq_mx_dequant.h"
namespace fq {
FQ_INSTANTIATE_MX_DEQUANT(F32)
FQ_INSTANTIATE_MX_DEQUANT(BF16)
FQ_INSTANTIATE_MX_DEQUANT(F16)
}
